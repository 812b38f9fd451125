"""Batched FourQ engine: a thin object over one fourq_ctx (one GPU, one HIP stream).

Array conventions are the C ABI's (include/fourq_amd.h): uint64 little-endian words,
scalars (n,4), affine points (n,8), R1 points (n,20), tables (128,).  Host entry points take and
return numpy arrays; the `*_dev` entry points take device pointers (ints, or anything with a
`data_ptr()` such as a torch tensor), enqueue on the engine's stream and do not synchronise.
"""
import ctypes
import os
import threading

import numpy as np

from . import _lib
from ._lib import PRIM, FourQError, HostStats, check


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        return ctypes.c_void_p(x.data_ptr())
    raise TypeError("expected a pointer, numpy array or tensor, got %r" % type(x))


def _host(a, cols, dtype=np.uint64):
    a = np.ascontiguousarray(a, dtype=dtype)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


def _out(out, n, cols, dtype=np.uint64):
    """A caller-provided result array (e.g. a row slice of a bigger one, or pinned memory from host_empty) or a fresh one."""
    shape = (n,) if cols is None else (n, cols)
    if out is None:
        return np.empty(shape, dtype=dtype)
    if out.dtype != dtype or out.shape != shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous %s %s array" % (shape, np.dtype(dtype).name))
    return out


class Engine:
    def __init__(self, device=None, stream=None):
        self._lib = _lib.load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        ctx = ctypes.c_void_p()
        check(self._lib.fourq_ctx_create(int(device), ctypes.byref(ctx)))
        self._ctx = ctx
        self.device = int(device)
        if stream is not None:
            self.set_stream(stream)

        self._pinned = {}            # address -> size of the pinned host blocks handed out by host_empty()

    # ---- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            for addr in list(getattr(self, "_pinned", {})):
                self._lib.fourq_host_free(self._ctx, ctypes.c_void_p(addr))
            self._pinned = {}
            self._lib.fourq_ctx_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        check(rc, self._ctx)

    def set_stream(self, stream):
        """`stream`: a hipStream_t as int (e.g. torch.cuda.current_stream().cuda_stream) or None."""
        handle = getattr(stream, "cuda_stream", stream)
        self._ck(self._lib.fourq_ctx_set_stream(self._ctx, ctypes.c_void_p(handle) if handle else None))

    def sync(self):
        self._ck(self._lib.fourq_ctx_sync(self._ctx))

    @property
    def ct_select(self):
        """Constant-time table selection (fourq_ctx_set_ct_select): False by default -- the digit is an address, as in
        the reference; True reads the whole table at every step.  Results are identical."""
        on = ctypes.c_int()
        self._ck(self._lib.fourq_ctx_get_ct_select(self._ctx, ctypes.byref(on)))
        return bool(on.value)

    @ct_select.setter
    def ct_select(self, on):
        self._ck(self._lib.fourq_ctx_set_ct_select(self._ctx, 1 if on else 0))

    # ---- pinned host memory (the fast path of the host-pointer calls) ---------------------------
    def host_empty(self, shape, dtype=np.uint64):
        """Uninitialised numpy array in pinned host memory (fourq_host_alloc): the host-array entry points move such
        arrays by DMA without a bounce copy.  The memory belongs to the engine and is released by close() (or
        host_free); arrays must not be used after that."""
        dt = np.dtype(dtype)
        count = int(np.prod(shape, dtype=np.int64)) if np.ndim(shape) else int(shape)
        nbytes = max(16, count * dt.itemsize)
        ptr = ctypes.c_void_p()
        self._ck(self._lib.fourq_host_alloc(self._ctx, nbytes, ctypes.byref(ptr)))
        self._pinned[ptr.value] = nbytes
        buf = (ctypes.c_char * nbytes).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)

    def host_array(self, a, dtype=None):
        """Copy of `a` in pinned host memory."""
        a = np.asarray(a, dtype=dtype)
        out = self.host_empty(a.shape, a.dtype)
        out[...] = a
        return out

    def host_free(self, a):
        addr = a.ctypes.data
        if addr in self._pinned:
            self._ck(self._lib.fourq_host_free(self._ctx, ctypes.c_void_p(addr)))
            del self._pinned[addr]

    def host_timing(self, on):
        """Time the chunk copies of the following host-array calls (fourq_ctx_set_host_timing): `host_stats()` then reports h2d_ms /
        d2h_ms and the GB/s they imply.  Off by default -- the event records are not free."""
        self._ck(self._lib.fourq_ctx_set_host_timing(self._ctx, 1 if on else 0))

    def diag_clock(self, window_us=20000):
        """Shader clock in MHz the device holds right now, measured inside a kernel over `window_us` (fourq_diag_clock): dict with median,
        min, max over the probe's 16 waves and `under_load` (the engine's stream still had work in flight when the window closed).  Call
        it with work queued on the engine's stream for longer than the window."""
        med, lo, hi, busy = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self._ck(self._lib.fourq_diag_clock(self._ctx, int(window_us), ctypes.byref(med), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(busy)))
        return {"mhz": med.value, "mhz_min": lo.value, "mhz_max": hi.value, "window_us": int(window_us), "under_load": bool(busy.value)}

    def diag_clock_begin(self):
        """First stamp of a clock bracket, enqueued on the engine's stream (fourq_diag_clock_begin): the clock reported by diag_clock_end()
        is that of everything enqueued between this and diag_clock_stop()."""
        self._ck(self._lib.fourq_diag_clock_begin(self._ctx))

    def diag_clock_stop(self):
        """Second stamp, enqueued behind the bracketed work (fourq_diag_clock_stop); the host does not wait."""
        self._ck(self._lib.fourq_diag_clock_stop(self._ctx))

    def diag_clock_end(self):
        med, lo, hi, win = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._ck(self._lib.fourq_diag_clock_end(self._ctx, ctypes.byref(med), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(win)))
        return {"mhz": med.value, "mhz_min": lo.value, "mhz_max": hi.value, "window_us": win.value}

    def host_stats(self):
        """Transfer statistics of the last host-array call: bytes, chunks, pinned flags; copy milliseconds and GB/s under host_timing(True)."""
        st = HostStats()
        self._ck(self._lib.fourq_ctx_host_stats(self._ctx, ctypes.byref(st)))
        d = {f: getattr(st, f) for f, _ in HostStats._fields_}
        d["gbs_h2d"] = st.h2d_bytes / st.h2d_ms / 1e6 if st.h2d_ms > 0 else None
        d["gbs_d2h"] = st.d2h_bytes / st.d2h_ms / 1e6 if st.d2h_ms > 0 else None
        return d

    def host_chunk_stamps(self):
        """Per chunk of the last host-array call made under host_timing(True): [copy-in start, copy-in end, copy-out start, copy-out end,
        kernels start, kernels end] in ms since the call's first event (fourq_ctx_host_chunk_stamps)."""
        rows, buf = [], (ctypes.c_double * 6)()
        while self._lib.fourq_ctx_host_chunk_stamps(self._ctx, len(rows), buf) == 0:
            rows.append(list(buf))
        return rows

    def reserve(self, n):
        """Size the context's internal buffers for `*_dev` batches of up to n elements (fourq_ctx_reserve): such calls then
        only enqueue -- no hidden stream synchronisation, capturable into a HIP graph."""
        self._ck(self._lib.fourq_ctx_reserve(self._ctx, int(n)))

    @property
    def build_id(self):
        return self._lib.fourq_build_id().decode()

    @property
    def version(self):
        return int(self._lib.fourq_version())

    @property
    def lanes(self):
        n = ctypes.c_size_t()
        self._ck(self._lib.fourq_ctx_lanes(self._ctx, ctypes.byref(n)))
        return n.value

    # ---- tables ----------------------------------------------------------------------------
    def _table(self, fn, p_r1):
        p = _host(p_r1, None).ravel()
        if p.size != 20:
            raise ValueError("an R1 point is 20 words")
        out = np.empty(128, dtype=np.uint64)
        self._ck(fn(self._ctx, _ptr(p), _ptr(out)))
        return out

    def table_endo(self, p_r1):
        return self._table(self._lib.fourq_table_endo, p_r1)

    def table_windowed(self, p_r1):
        return self._table(self._lib.fourq_table_windowed, p_r1)

    # ---- scalar multiplication (host arrays) -----------------------------------------------
    def _mul(self, fn, scalars, second, second_cols, out=None):
        s = _host(scalars, 4)
        b = _host(second, second_cols)
        if second_cols == 20 and len(b) != len(s):
            raise ValueError("scalars and points differ in length")
        if second_cols is None and b.size != 128:
            raise ValueError("a table is 128 words")
        out = _out(out, len(s), 20)
        self._ck(fn(self._ctx, _ptr(s), _ptr(b), _ptr(out), len(s)))
        return out

    # `out`: optional preallocated result array, e.g. from host_empty() (pinned: no bounce copy on the way back)
    def mul_endo(self, scalars, points_r1, out=None):
        return self._mul(self._lib.fourq_mul_endo_batch, scalars, points_r1, 20, out)

    def mul_windowed(self, scalars, points_r1, out=None):
        return self._mul(self._lib.fourq_mul_windowed_batch, scalars, points_r1, 20, out)

    def mul_affine(self, scalars, points_affine, kind="endo", out=None):
        """R1toAffine(MUL_<kind>(m_i, AffineToR1(P_i))) (curve4q.py:100-106): affine in, canonical affine out -- 160 bytes per
        operation across the link instead of the raw-R1 form's 352 (fourq_mul_*_affine_batch)."""
        s, p = _host(scalars, 4), _host(points_affine, 8)
        if len(s) != len(p):
            raise ValueError("scalars and points differ in length")
        out = _out(out, len(s), 8)
        fn = self._lib.fourq_mul_endo_affine_batch if kind == "endo" else self._lib.fourq_mul_windowed_affine_batch
        self._ck(fn(self._ctx, _ptr(s), _ptr(p), _ptr(out), len(s)))
        return out

    def mul_bytes(self, scalars, points32, kind="endo", out=None, status=None):
        """encode(R1toAffine(MUL_<kind>(m_i, AffineToR1(decode(B_i))))) (curve4q.py:41-96): 32-byte points in and out, 96 bytes per
        operation (fourq_mul_*_bytes_batch).  Returns ((n, 32) uint8, status): 0 ok, 16 + decode status."""
        s, b = _host(scalars, 4), _host(points32, 32, np.uint8)
        if len(s) != len(b):
            raise ValueError("scalars and points differ in length")
        out, status = _out(out, len(s), 32, np.uint8), _out(status, len(s), None, np.uint8)
        fn = self._lib.fourq_mul_endo_bytes_batch if kind == "endo" else self._lib.fourq_mul_windowed_bytes_batch
        self._ck(fn(self._ctx, _ptr(s), _ptr(b), _ptr(out), _ptr(status), len(s)))
        return out, status

    def mul_affine_dev(self, scalars, points_affine, out_affine, n, kind="endo"):
        fn = self._lib.fourq_mul_endo_affine_batch_dev if kind == "endo" else self._lib.fourq_mul_windowed_affine_batch_dev
        self._ck(fn(self._ctx, _ptr(scalars), _ptr(points_affine), _ptr(out_affine), n))

    def mul_bytes_dev(self, scalars, points32, out32, status, n, kind="endo"):
        fn = self._lib.fourq_mul_endo_bytes_batch_dev if kind == "endo" else self._lib.fourq_mul_windowed_bytes_batch_dev
        self._ck(fn(self._ctx, _ptr(scalars), _ptr(points32), _ptr(out32), _ptr(status), n))

    def mul_endo_fixed(self, scalars, table, out=None):
        return self._mul(self._lib.fourq_mul_endo_fixed_batch, scalars, table, None, out)

    def mul_windowed_fixed(self, scalars, table, out=None):
        return self._mul(self._lib.fourq_mul_windowed_fixed_batch, scalars, table, None, out)

    def mul_endo_mixed(self, scalars, points_r1, flags, table, out=None):
        s, p = _host(scalars, 4), _host(points_r1, 20)
        f = _host(flags, None, np.uint8).ravel()
        t = _host(table, None).ravel()
        if not (len(s) == len(p) == len(f)) or t.size != 128:
            raise ValueError("mixed batch: inconsistent shapes")
        out = _out(out, len(s), 20)
        self._ck(self._lib.fourq_mul_endo_mixed_batch(self._ctx, _ptr(s), _ptr(p), _ptr(f), _ptr(t), _ptr(out), len(s)))
        return out

    # ---- Diffie-Hellman ----------------------------------------------------------------------
    def _dh(self, fn, scalars, points_affine, table, out=None, status=None):
        s, p = _host(scalars, 4), _host(points_affine, 8)
        if len(s) != len(p):
            raise ValueError("scalars and points differ in length")
        t = None if table is None else _host(table, None).ravel()
        if t is not None and t.size != 128:
            raise ValueError("a table is 128 words")
        out, status = _out(out, len(s), 8), _out(status, len(s), None, np.uint8)
        self._ck(fn(self._ctx, _ptr(s), _ptr(p), _ptr(t), _ptr(out), _ptr(status), len(s)))
        return out, status

    def dh_endo(self, scalars, points_affine, table=None, out=None, status=None):
        return self._dh(self._lib.fourq_dh_endo_batch, scalars, points_affine, table, out, status)

    def dh_windowed(self, scalars, points_affine, table=None, out=None, status=None):
        return self._dh(self._lib.fourq_dh_windowed_batch, scalars, points_affine, table, out, status)

    def dh_exchange(self, a_scalars, b_scalars, base_affine, table392=None, out=None, status=None):
        """One exchange per row: DH_endo(a_i, DH_endo(b_i, base)) (curve4q.py:731), the first half's
        public keys staying on the device (fourq_dh_exchange_batch).

        `table392` = table_endo([392]base) makes the first half fixed-base.  Returns (affine, status):
        status is the first failure of either half."""
        a, b = _host(a_scalars, 4), _host(b_scalars, 4)
        if len(a) != len(b):
            raise ValueError("the two scalar arrays differ in length")
        base = _host(base_affine, None).ravel()
        if base.size != 8:
            raise ValueError("an affine point is 8 words")
        t = None if table392 is None else _host(table392, None).ravel()
        if t is not None and t.size != 128:
            raise ValueError("a table is 128 words")
        out, status = _out(out, len(a), 8), _out(status, len(a), None, np.uint8)
        self._ck(self._lib.fourq_dh_exchange_batch(self._ctx, _ptr(a), _ptr(b), _ptr(base), _ptr(t), _ptr(out), _ptr(status), len(a)))
        return out, status

    def dh_exchange_comb(self, a_scalars, b_scalars, comb=None, out=None, status=None):
        """One exchange per row with the key-generation half through the comb of [392]base (fourq_dh_exchange_comb_batch):
        DH_endo(a_i, DH_endo(b_i, base)) -- same outputs as dh_exchange, the first half 3x cheaper.  `comb`: a comb table
        (comb_table([392]base)) or None = the table staged by comb_stage().  Returns (affine, status)."""
        a, b = _host(a_scalars, 4), _host(b_scalars, 4)
        if len(a) != len(b):
            raise ValueError("the two scalar arrays differ in length")
        t = None
        if comb is not None:
            t = _host(comb, None).ravel()
            if t.size != _lib.COMB_WORDS:
                raise ValueError("a comb table is %d words" % _lib.COMB_WORDS)
        out, status = _out(out, len(a), 8), _out(status, len(a), None, np.uint8)
        self._ck(self._lib.fourq_dh_exchange_comb_batch(self._ctx, _ptr(a), _ptr(b), _ptr(t), _ptr(out), _ptr(status), len(a)))
        return out, status

    def dh_exchange_comb_dev(self, a_scalars, b_scalars, comb_host, out_affine, status, n):
        t = None if comb_host is None else _host(comb_host, None).ravel()
        self._ck(self._lib.fourq_dh_exchange_comb_batch_dev(self._ctx, _ptr(a_scalars), _ptr(b_scalars), _ptr(t), _ptr(out_affine), _ptr(status), n))

    # ---- [k]B + [l]P and signature checks (fourq_double_mul_* / fourq_verify_bytes_*) ----------------
    def _comb_arg(self, comb):
        if comb is None:
            return None
        t = _host(comb, None).ravel()
        if t.size != _lib.COMB_WORDS:
            raise ValueError("a comb table is %d words" % _lib.COMB_WORDS)
        return t

    def double_mul(self, k_scalars, l_scalars, points_affine, comb=None, out=None):
        """Canonical affine [k_i]B + [l_i]P_i, (n, 8) words: B the base of `comb` (comb_table(B), B of order N; None = the table
        staged by comb_stage()), P_i affine.  Checks nothing, like MUL_*; the neutral point (0, 1) is an ordinary result."""
        k, l, p = _host(k_scalars, 4), _host(l_scalars, 4), _host(points_affine, 8)
        if not len(k) == len(l) == len(p):
            raise ValueError("the scalar and point arrays differ in length")
        out = _out(out, len(k), 8)
        self._ck(self._lib.fourq_double_mul_affine_batch(self._ctx, _ptr(k), _ptr(self._comb_arg(comb)), _ptr(l), _ptr(p), _ptr(out), len(k)))
        return out

    def double_mul_bytes(self, k_scalars, l_scalars, points32, comb=None, out=None, status=None):
        """encode([k_i]B + [l_i]decode(points32[i])): ((n, 32) bytes, status); status[i] = 0 or BYTES_DECODE_BASE + DECODE_*."""
        k, l, p = _host(k_scalars, 4), _host(l_scalars, 4), _host(points32, 32, np.uint8)
        if not len(k) == len(l) == len(p):
            raise ValueError("the scalar and point arrays differ in length")
        out, status = _out(out, len(k), 32, np.uint8), _out(status, len(k), None, np.uint8)
        self._ck(self._lib.fourq_double_mul_bytes_batch(self._ctx, _ptr(k), _ptr(self._comb_arg(comb)), _ptr(l), _ptr(p), _ptr(out), _ptr(status), len(k)))
        return out, status

    def verify_bytes(self, k_scalars, l_scalars, keys32, expect32, comb=None, ok=None, status=None):
        """The curve part of a Schnorr-type verification: ok[i] = 1 iff keys32[i] decodes and encode([k_i]B + [l_i]decode(keys32[i]))
        equals expect32[i] byte for byte.  Returns (ok, status): status says why a 0 is a 0 (non-zero = the key did not decode).
        For SchnorrQ: verify_bytes(s, h, A32, R32) with h = H(R, A, msg) hashed by the caller and `comb` the table of the generator."""
        k, l = _host(k_scalars, 4), _host(l_scalars, 4)
        a, e = _host(keys32, 32, np.uint8), _host(expect32, 32, np.uint8)
        if not len(k) == len(l) == len(a) == len(e):
            raise ValueError("the scalar, key and expectation arrays differ in length")
        ok, status = _out(ok, len(k), None, np.uint8), _out(status, len(k), None, np.uint8)
        self._ck(self._lib.fourq_verify_bytes_batch(self._ctx, _ptr(k), _ptr(self._comb_arg(comb)), _ptr(l), _ptr(a), _ptr(e), _ptr(ok), _ptr(status), len(k)))
        return ok, status

    def double_mul_dev(self, k_scalars, l_scalars, points_affine, out_affine, n, comb_host=None):
        self._ck(self._lib.fourq_double_mul_affine_batch_dev(self._ctx, _ptr(k_scalars), _ptr(self._comb_arg(comb_host)), _ptr(l_scalars), _ptr(points_affine), _ptr(out_affine), n))

    def double_mul_bytes_dev(self, k_scalars, l_scalars, points32, out32, status, n, comb_host=None):
        self._ck(self._lib.fourq_double_mul_bytes_batch_dev(self._ctx, _ptr(k_scalars), _ptr(self._comb_arg(comb_host)), _ptr(l_scalars), _ptr(points32), _ptr(out32), _ptr(status), n))

    def verify_bytes_dev(self, k_scalars, l_scalars, keys32, expect32, ok, status, n, comb_host=None):
        self._ck(self._lib.fourq_verify_bytes_batch_dev(self._ctx, _ptr(k_scalars), _ptr(self._comb_arg(comb_host)), _ptr(l_scalars), _ptr(keys32), _ptr(expect32), _ptr(ok), _ptr(status), n))

    # ---- grouped multi-scalar multiplication (fourq_msm_*): out[g] = sum_j [k_gj]P_gj over groups of one length ----------------
    @staticmethod
    def _groups(n, group_size):
        group_size = int(group_size)
        if group_size <= 0:
            raise ValueError("group_size must be positive")
        if n % group_size:
            raise ValueError("%d elements are not a whole number of groups of %d" % (n, group_size))
        return n // group_size, group_size

    def msm(self, scalars, points_affine, group_size, out=None):
        """Canonical affine sums, (n // group_size, 8) words: out[g] = sum of [k_i]P_i over the group_size elements of group g, laid out
        group after group.  Checks nothing, like MUL_*; the neutral point (0, 1) is an ordinary result.  Ragged groups: msm_ragged, or pad with scalar 0."""
        k, p = _host(scalars, 4), _host(points_affine, 8)
        if len(k) != len(p):
            raise ValueError("the scalar and point arrays differ in length")
        groups, group_size = self._groups(len(k), group_size)
        out = _out(out, groups, 8)
        self._ck(self._lib.fourq_msm_affine_batch(self._ctx, _ptr(k), _ptr(p), _ptr(out), groups, group_size))
        return out

    def msm_bytes(self, scalars, points32, group_size, out=None, status=None):
        """encode(sum of [k_i]decode(points32[i])) per group: ((n // group_size, 32) bytes, status); status[g] = 0 or BYTES_DECODE_BASE +
        the largest DECODE_* among the group's elements (out[g] is zero then; decode() tells which element it was)."""
        k, p = _host(scalars, 4), _host(points32, 32, np.uint8)
        if len(k) != len(p):
            raise ValueError("the scalar and point arrays differ in length")
        groups, group_size = self._groups(len(k), group_size)
        out, status = _out(out, groups, 32, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_msm_bytes_batch(self._ctx, _ptr(k), _ptr(p), _ptr(out), _ptr(status), groups, group_size))
        return out, status

    def msm_dev(self, scalars, points_affine, out_affine, groups, group_size):
        self._ck(self._lib.fourq_msm_affine_batch_dev(self._ctx, _ptr(scalars), _ptr(points_affine), _ptr(out_affine), groups, group_size))

    def msm_bytes_dev(self, scalars, points32, out32, status, groups, group_size):
        self._ck(self._lib.fourq_msm_bytes_batch_dev(self._ctx, _ptr(scalars), _ptr(points32), _ptr(out32), _ptr(status), groups, group_size))

    # ---- ragged grouped sums (fourq_raggedsum_*): the same sums over groups of any length, 0 included, by a shape the context holds -----
    # offsets: groups + 1 ascending row offsets from 0; group g owns rows offsets[g] .. offsets[g + 1] - 1.
    @staticmethod
    def _offsets(offsets):
        a = np.asarray(offsets)
        if a.ndim != 1 or len(a) < 2 or a.dtype.kind not in "iu" or (a < 0).any() or (a > 0xffffffff).any():
            raise ValueError("offsets must be groups + 1 >= 2 row offsets that fit 32 bits")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def msm_shape(self, offsets):
        """Install the shape (fourq_raggedsum_shape_set): validated and planned on the host, its descriptors uploaded.  Replaces the old
        shape once the new one is complete; an invalid one (offsets[0] != 0, a descending pair, too many rows) raises and the old one stays."""
        a = self._offsets(offsets)
        self._ck(self._lib.fourq_raggedsum_shape_set(self._ctx, _ptr(a), len(a) - 1))
        self._shape = a.copy()

    def msm_shape_count(self):
        """(groups, rows) of the installed shape, (0, 0) when none was ever set."""
        groups, rows = ctypes.c_size_t(), ctypes.c_size_t()
        self._ck(self._lib.fourq_raggedsum_shape_count(self._ctx, ctypes.byref(groups), ctypes.byref(rows)))
        return int(groups.value), int(rows.value)

    def msm_shape_reserve(self):
        """Size the work buffer for the installed shape (fourq_raggedsum_shape_reserve; reserve() is not enough): the `_dev` calls then
        only enqueue."""
        self._ck(self._lib.fourq_raggedsum_shape_reserve(self._ctx))

    def _ragged(self, offsets, n):
        """(groups, rows) of the shape a call runs on: `offsets` installed first unless it equals the one this Engine installed last"""
        if offsets is not None:
            a = self._offsets(offsets)
            last = getattr(self, "_shape", None)
            if last is None or not np.array_equal(last, a):
                self.msm_shape(a)
        groups, rows = self.msm_shape_count()
        if groups and n != rows:
            raise ValueError("%d elements, but the shape has %d rows" % (n, rows))
        return groups

    def msm_ragged(self, scalars, points_affine, offsets=None, out=None):
        """Canonical affine sums, (groups, 8) words: out[g] = sum of [k_i]P_i over the rows of group g; an empty group gives the neutral
        (0, 1).  offsets=None runs on the installed shape.  Byte for byte msm() on each group alone."""
        k, p = _host(scalars, 4), _host(points_affine, 8)
        if len(k) != len(p):
            raise ValueError("the scalar and point arrays differ in length")
        groups = self._ragged(offsets, len(k))
        out = _out(out, groups, 8)
        self._ck(self._lib.fourq_raggedsum_affine(self._ctx, _ptr(k), _ptr(p), _ptr(out)))
        return out

    def msm_ragged_bytes(self, scalars, points32, offsets=None, out=None, status=None):
        """encode(sum of [k_i]decode(points32[i])) per group: ((groups, 32) bytes, status); status[g] = 0 or BYTES_DECODE_BASE + the largest
        DECODE_* among the group's rows (out[g] is zero then).  An empty group gives 01 00 .. 00 with status 0."""
        k, p = _host(scalars, 4), _host(points32, 32, np.uint8)
        if len(k) != len(p):
            raise ValueError("the scalar and point arrays differ in length")
        groups = self._ragged(offsets, len(k))
        out, status = _out(out, groups, 32, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_raggedsum_bytes(self._ctx, _ptr(k), _ptr(p), _ptr(out), _ptr(status)))
        return out, status

    def msm_ragged_dev(self, scalars, points_affine, out_affine):
        self._ck(self._lib.fourq_raggedsum_affine_dev(self._ctx, _ptr(scalars), _ptr(points_affine), _ptr(out_affine)))

    def msm_ragged_bytes_dev(self, scalars, points32, out32, status):
        self._ck(self._lib.fourq_raggedsum_bytes_dev(self._ctx, _ptr(scalars), _ptr(points32), _ptr(out32), _ptr(status)))

    # ---- the same sums by the bucket method (fourq_bucketsum_*): same arrays, same bytes, for large groups ----------------------------
    # window: 0 = the library picks (bucket_sum_window; the ladder route where no window beat it), 4..12 = the bucket route with that window.
    # With ct_select on the ladder route runs whatever the window is (a bucket's address is a digit of a scalar).
    def bucket_sum_window(self, group_size):
        """What window=0 stands for at this group size: 0 (the ladder route, msm) or 4..12."""
        return int(self._lib.fourq_bucketsum_window(int(group_size)))

    def bucket_sum_reserve(self, groups, group_size, window=0):
        """Size the work buffer for `bucket_sum*_dev` calls of this shape and window (fourq_bucketsum_reserve; reserve() is not enough
        for them): such calls then only enqueue."""
        self._ck(self._lib.fourq_bucketsum_reserve(self._ctx, int(groups), int(group_size), int(window)))

    def bucket_sum(self, scalars, points_affine, group_size, window=0, out=None):
        """msm()'s result, byte for byte, by the bucket method."""
        k, p = _host(scalars, 4), _host(points_affine, 8)
        if len(k) != len(p):
            raise ValueError("the scalar and point arrays differ in length")
        groups, group_size = self._groups(len(k), group_size)
        out = _out(out, groups, 8)
        self._ck(self._lib.fourq_bucketsum_affine(self._ctx, _ptr(k), _ptr(p), _ptr(out), groups, group_size, int(window)))
        return out

    def bucket_sum_bytes(self, scalars, points32, group_size, window=0, out=None, status=None):
        """msm_bytes()'s (out32, status), byte for byte, by the bucket method."""
        k, p = _host(scalars, 4), _host(points32, 32, np.uint8)
        if len(k) != len(p):
            raise ValueError("the scalar and point arrays differ in length")
        groups, group_size = self._groups(len(k), group_size)
        out, status = _out(out, groups, 32, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_bucketsum_bytes(self._ctx, _ptr(k), _ptr(p), _ptr(out), _ptr(status), groups, group_size, int(window)))
        return out, status

    def bucket_sum_dev(self, scalars, points_affine, out_affine, groups, group_size, window=0):
        self._ck(self._lib.fourq_bucketsum_affine_dev(self._ctx, _ptr(scalars), _ptr(points_affine), _ptr(out_affine), groups, group_size, int(window)))

    def bucket_sum_bytes_dev(self, scalars, points32, out32, status, groups, group_size, window=0):
        self._ck(self._lib.fourq_bucketsum_bytes_dev(self._ctx, _ptr(scalars), _ptr(points32), _ptr(out32), _ptr(status), groups, group_size, int(window)))

    # ---- commitments over a fixed generator set (fourq_commit_*): out[g] = sum_j [k_gj]B_j, one comb per generator held by the context ----
    # route: 0 = the library picks by the number of groups (commit_route), 1 = staged (comb j in a CU's LDS), 2 = gather (entries read where
    # they lie).  With ct_select on the route makes no difference.  The bytes are the same on every route.
    def commit_generators(self, count, dst):
        """`count` generators nobody knows a relation between: hash_to_curve(I2OSP(j, 4), dst, affine=True) for j < count, (count, 8) words.
        They have order N by construction (the x392 chain)."""
        msgs = np.array([list(int(j).to_bytes(4, "big")) for j in range(int(count))], dtype=np.uint8).reshape(int(count), 4)
        return self.hash_to_curve(msgs, dst=dst, affine=True)

    def commit_bases(self, points_affine):
        """Build one comb per base on the device and keep the set in the context (fourq_commit_bases_set): (m, 8) affine words, 1 <= m <= 4096,
        every base of order N (not checked).  Replaces any earlier set; the staged comb and tables are untouched."""
        p = _host(points_affine, 8)
        self._ck(self._lib.fourq_commit_bases_set(self._ctx, _ptr(p), len(p)))

    @property
    def commit_bases_count(self):
        """The size of the generator set, 0 when none was ever set."""
        m = ctypes.c_size_t()
        self._ck(self._lib.fourq_commit_bases_count(self._ctx, ctypes.byref(m)))
        return int(m.value)

    def commit_route(self, groups):
        """What route=0 stands for at this number of groups: 1 (staged) or 2 (gather)."""
        return int(self._lib.fourq_commit_route(int(groups)))

    def commit_reserve(self, groups, group_size):
        """Size the work buffer for `commit*_dev` calls of at most this shape (reserve() is not enough for them): such calls then only enqueue."""
        self._ck(self._lib.fourq_commit_reserve(self._ctx, int(groups), int(group_size)))

    def commit(self, scalars, group_size, route=0, out=None):
        """Canonical affine commitments, (n // group_size, 8) words: out[g] = sum over j < group_size of [k_gj]B_j with the bases of
        commit_bases -- msm()'s result over the tiled bases, byte for byte.  The neutral point (0, 1) is an ordinary result."""
        k = _host(scalars, 4)
        groups, group_size = self._groups(len(k), group_size)
        out = _out(out, groups, 8)
        self._ck(self._lib.fourq_commit_affine(self._ctx, _ptr(k), _ptr(out), groups, group_size, int(route)))
        return out

    def commit_bytes(self, scalars, group_size, route=0, out=None):
        """encode() of commit()'s points: (n // group_size, 32) bytes; the neutral is 01 00 .. 00.  No status: nothing is decoded."""
        k = _host(scalars, 4)
        groups, group_size = self._groups(len(k), group_size)
        out = _out(out, groups, 32, np.uint8)
        self._ck(self._lib.fourq_commit_bytes(self._ctx, _ptr(k), _ptr(out), groups, group_size, int(route)))
        return out

    def commit_dev(self, scalars, out_affine, groups, group_size, route=0):
        self._ck(self._lib.fourq_commit_affine_dev(self._ctx, _ptr(scalars), _ptr(out_affine), groups, group_size, int(route)))

    def commit_bytes_dev(self, scalars, out32, groups, group_size, route=0):
        self._ck(self._lib.fourq_commit_bytes_dev(self._ctx, _ptr(scalars), _ptr(out32), groups, group_size, int(route)))

    # ---- signatures from bytes (fourq_sha512_* / fourq_sig_*): SHA-512 and the arithmetic modulo N run on the device -------------
    @staticmethod
    def _msgs(msgs, lens, n=None):
        """(matrix, stride, lens or None, msg_len): `msgs` a 2-D uint8 array, one message per row (row stride = its second dimension);
        `lens` the rows' lengths, or None = every row is used whole."""
        m = np.ascontiguousarray(msgs, dtype=np.uint8)
        if m.ndim != 2:
            raise ValueError("msgs must be a 2-D uint8 array, one message per row (codec.pack_messages makes one)")
        if n is not None and len(m) != n:
            raise ValueError("the message matrix and the other arrays differ in length")
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.uint32).ravel()
            if len(lens) != len(m):
                raise ValueError("lens must have one entry per message")
        return m, m.shape[1], lens, m.shape[1]

    def sha512(self, msgs, lens=None, out=None):
        """SHA-512 of every row of `msgs` (its first lens[i] bytes): (n, 64) uint8."""
        m, stride, lens, msg_len = self._msgs(msgs, lens)
        out = _out(out, len(m), 64, np.uint8)
        self._ck(self._lib.fourq_sha512_batch(self._ctx, _ptr(m) if stride else None, stride, _ptr(lens), msg_len, _ptr(out), len(m)))
        return out

    def sha512_dev(self, msgs, stride, lens, msg_len, out64, n):
        self._ck(self._lib.fourq_sha512_batch_dev(self._ctx, _ptr(msgs), stride, _ptr(lens), msg_len, _ptr(out64), n))

    def sig_keygen(self, sk32, comb=None, out=None):
        """Public keys encode([LE(SHA-512(sk)[0:32])]G), (n, 32) uint8, from (n, 32) secret keys.  `comb`: the comb of the generator
        (comb_table(AffineToR1(Gx, Gy))) or None = the table staged by comb_stage()."""
        sk = _host(sk32, 32, np.uint8)
        out = _out(out, len(sk), 32, np.uint8)
        self._ck(self._lib.fourq_sig_keygen_batch(self._ctx, _ptr(sk), _ptr(self._comb_arg(comb)), _ptr(out), len(sk)))
        return out

    def sig_keygen_dev(self, sk32, pk32, n, comb_host=None):
        self._ck(self._lib.fourq_sig_keygen_batch_dev(self._ctx, _ptr(sk32), _ptr(self._comb_arg(comb_host)), _ptr(pk32), n))

    def sig_sign(self, sk32, pk32, msgs, lens=None, comb=None, out=None):
        """Signatures R || s, (n, 64) uint8 (the scheme: include/fourq_amd.h).  pk32 is an input; it is not checked against sk32."""
        sk, pk = _host(sk32, 32, np.uint8), _host(pk32, 32, np.uint8)
        if len(sk) != len(pk):
            raise ValueError("the secret and public key arrays differ in length")
        m, stride, lens, msg_len = self._msgs(msgs, lens, len(sk))
        out = _out(out, len(sk), 64, np.uint8)
        self._ck(self._lib.fourq_sig_sign_batch(self._ctx, _ptr(sk), _ptr(pk), _ptr(self._comb_arg(comb)), _ptr(m) if stride else None, stride, _ptr(lens), msg_len,
                                                _ptr(out), len(sk)))
        return out

    def sig_sign_dev(self, sk32, pk32, msgs, stride, lens, msg_len, sig64, n, comb_host=None):
        self._ck(self._lib.fourq_sig_sign_batch_dev(self._ctx, _ptr(sk32), _ptr(pk32), _ptr(self._comb_arg(comb_host)), _ptr(msgs), stride, _ptr(lens), msg_len,
                                                    _ptr(sig64), n))

    def sig_verify(self, pk32, msgs, sig64, lens=None, comb=None, ok=None, status=None):
        """(ok, status) per row: ok[i] = 1 iff sig64[i] is a valid signature of msgs[i] under pk32[i].  status says why a 0 is a 0:
        0 = plain mismatch, _lib.SIG_S_RANGE = s >= N, _lib.BYTES_DECODE_BASE + DECODE_* = the key does not decode."""
        pk, sig = _host(pk32, 32, np.uint8), _host(sig64, 64, np.uint8)
        if len(pk) != len(sig):
            raise ValueError("the key and signature arrays differ in length")
        m, stride, lens, msg_len = self._msgs(msgs, lens, len(pk))
        ok, status = _out(ok, len(pk), None, np.uint8), _out(status, len(pk), None, np.uint8)
        self._ck(self._lib.fourq_sig_verify_batch(self._ctx, _ptr(pk), _ptr(self._comb_arg(comb)), _ptr(m) if stride else None, stride, _ptr(lens), msg_len,
                                                  _ptr(sig), _ptr(ok), _ptr(status), len(pk)))
        return ok, status

    def sig_verify_dev(self, pk32, msgs, stride, lens, msg_len, sig64, ok, status, n, comb_host=None):
        self._ck(self._lib.fourq_sig_verify_batch_dev(self._ctx, _ptr(pk32), _ptr(self._comb_arg(comb_host)), _ptr(msgs), stride, _ptr(lens), msg_len,
                                                      _ptr(sig64), _ptr(ok), _ptr(status), n))

    # ---- signatures of registered keys (fourq_keyset_*, fourq_keyset_sig_verify*): rows name their public key by index, and the context
    # holds one comb per key (155 KiB each), so [s]G + [h]A_id is two combs in one accumulator instead of a comb and a ladder --------------
    def keyset_set(self, keys32):
        """Register (m, 32) public keys, 1 <= m <= 4096, replacing any earlier set; synchronous.  Returns one status byte per slot:
        0 = accepted, _lib.BYTES_DECODE_BASE + DECODE_* = does not decode, _lib.KEYSET_NOT_ORDER_N = decodes to a point outside the
        subgroup of order N.  A refused key keeps its slot; rows that name it are reported with its status."""
        pk = _host(keys32, 32, np.uint8)
        status = np.zeros(len(pk), dtype=np.uint8)
        self._ck(self._lib.fourq_keyset_set(self._ctx, _ptr(pk), len(pk), _ptr(status)))
        return status

    def keyset_count(self):
        """The number of registered keys; 0 when none were."""
        m = ctypes.c_size_t(0)
        self._ck(self._lib.fourq_keyset_count(self._ctx, ctypes.byref(m)))
        return int(m.value)

    def keyset_reserve(self, n):
        """Size the buffers for keyed `_dev` calls of at most n rows (reserve() is not enough for them): such calls then only enqueue."""
        self._ck(self._lib.fourq_keyset_reserve(self._ctx, int(n)))

    def keyset_double_mul_bytes(self, k_scalars, l_scalars, ids, comb=None, out=None, status=None):
        """encode([k_i]B + [l_i]A_ids[i]) over the registered keys: ((n, 32) bytes, status).  status[i] = 0 or the key's own status (the
        row is zero then); an index outside the set is an error."""
        k, l, i = _host(k_scalars, 4), _host(l_scalars, 4), np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        if not len(k) == len(l) == len(i):
            raise ValueError("the scalar and index arrays differ in length")
        out, status = _out(out, len(k), 32, np.uint8), _out(status, len(k), None, np.uint8)
        self._ck(self._lib.fourq_keyset_double_mul_bytes(self._ctx, _ptr(k), _ptr(self._comb_arg(comb)), _ptr(l), _ptr(i), _ptr(out), _ptr(status), len(k)))
        return out, status

    def keyset_double_mul_bytes_dev(self, k_scalars, l_scalars, ids, out32, status, n, comb_host=None):
        self._ck(self._lib.fourq_keyset_double_mul_bytes_dev(self._ctx, _ptr(k_scalars), _ptr(self._comb_arg(comb_host)), _ptr(l_scalars), _ptr(ids), _ptr(out32),
                                                             _ptr(status), n))

    def sig_verify_keyed(self, ids, msgs, sig64, lens=None, comb=None, ok=None, status=None):
        """sig_verify() with pk32[i] = the registered key ids[i]: (ok, status).  status as sig_verify's, or the key's own status."""
        i, sig = np.ascontiguousarray(ids, dtype=np.uint32).ravel(), _host(sig64, 64, np.uint8)
        if len(i) != len(sig):
            raise ValueError("the index and signature arrays differ in length")
        m, stride, lens, msg_len = self._msgs(msgs, lens, len(i))
        ok, status = _out(ok, len(i), None, np.uint8), _out(status, len(i), None, np.uint8)
        self._ck(self._lib.fourq_keyset_sig_verify(self._ctx, _ptr(i), _ptr(self._comb_arg(comb)), _ptr(m) if stride else None, stride, _ptr(lens), msg_len,
                                                        _ptr(sig), _ptr(ok), _ptr(status), len(i)))
        return ok, status

    def sig_verify_keyed_dev(self, ids, msgs, stride, lens, msg_len, sig64, ok, status, n, comb_host=None):
        self._ck(self._lib.fourq_keyset_sig_verify_dev(self._ctx, _ptr(ids), _ptr(self._comb_arg(comb_host)), _ptr(msgs), stride, _ptr(lens), msg_len,
                                                            _ptr(sig64), _ptr(ok), _ptr(status), n))

    # ---- bytes to a point (fourq_hash_to_*: RFC 9380 with SHA-512 XMD, Elligator 2 and the x392 chain, include/fourq_amd.h) --------
    @staticmethod
    def _h2c(dst, mode):
        """(DST as a ctypes buffer, its length, FOURQ_H2C_*); a DST of 0 or more than 255 bytes is the library's FOURQ_ERR_INVALID."""
        dst = bytes(dst)
        modes = {"ro": _lib.H2C_RO, "nu": _lib.H2C_NU, _lib.H2C_RO: _lib.H2C_RO, _lib.H2C_NU: _lib.H2C_NU}
        if mode not in modes:
            raise ValueError('mode must be "ro" or "nu"')
        return ctypes.create_string_buffer(dst, max(len(dst), 1)), len(dst), modes[mode]

    def hash_to_field(self, msgs, lens=None, dst=b"", mode="ro", out=None):
        """u_0 [, u_1] of every row of `msgs`: (n, count, 4) uint64 canonical words, count = 2 ("ro") or 1 ("nu")."""
        buf, dst_len, mode = self._h2c(dst, mode)
        m, stride, lens, msg_len = self._msgs(msgs, lens)
        count = 2 if mode == _lib.H2C_RO else 1
        out = _out(out, len(m), 4 * count).reshape(len(m), count, 4)
        self._ck(self._lib.fourq_hash_to_field_batch(self._ctx, buf, dst_len, mode, _ptr(m) if stride else None, stride, _ptr(lens), msg_len, _ptr(out), len(m)))
        return out

    def hash_to_field_dev(self, msgs, stride, lens, msg_len, out_u, n, dst=b"", mode="ro"):
        buf, dst_len, mode = self._h2c(dst, mode)
        self._ck(self._lib.fourq_hash_to_field_batch_dev(self._ctx, buf, dst_len, mode, _ptr(msgs), stride, _ptr(lens), msg_len, _ptr(out_u), n))

    def map_to_curve(self, u, out=None):
        """Elligator 2 + the rational map of every u (n, 4) -- each coordinate any value below 2^128 -- as affine points (n, 8);
        no cofactor clearing."""
        u = _host(u, 4)
        out = _out(out, len(u), 8)
        self._ck(self._lib.fourq_map_to_curve_batch(self._ctx, _ptr(u), _ptr(out), len(u)))
        return out

    def map_to_curve_dev(self, u, out_affine, n):
        self._ck(self._lib.fourq_map_to_curve_batch_dev(self._ctx, _ptr(u), _ptr(out_affine), n))

    def hash_to_curve(self, msgs, lens=None, dst=b"", mode="ro", affine=False, out=None):
        """The point every row of `msgs` hashes to under the domain separation tag `dst` (1..255 bytes): (n, 32) uint8 encodings, or
        (n, 8) uint64 affine words with `affine`.  mode "ro": [392](map(u_0) + map(u_1)); "nu": [392]map(u_0)."""
        buf, dst_len, mode = self._h2c(dst, mode)
        m, stride, lens, msg_len = self._msgs(msgs, lens)
        out = _out(out, len(m), 8) if affine else _out(out, len(m), 32, np.uint8)
        fn = self._lib.fourq_hash_to_curve_affine_batch if affine else self._lib.fourq_hash_to_curve_batch
        self._ck(fn(self._ctx, buf, dst_len, mode, _ptr(m) if stride else None, stride, _ptr(lens), msg_len, _ptr(out), len(m)))
        return out

    def hash_to_curve_dev(self, msgs, stride, lens, msg_len, out, n, dst=b"", mode="ro", affine=False):
        buf, dst_len, mode = self._h2c(dst, mode)
        fn = self._lib.fourq_hash_to_curve_affine_batch_dev if affine else self._lib.fourq_hash_to_curve_batch_dev
        self._ck(fn(self._ctx, buf, dst_len, mode, _ptr(msgs), stride, _ptr(lens), msg_len, _ptr(out), n))

    # ---- oblivious PRF (fourq_oprf_*: blind, evaluate, finalize and the key holder's direct evaluation, include/fourq_amd.h) -------
    @staticmethod
    def _key(key):
        k = _host(key, None).ravel()
        if k.size != 4:
            raise ValueError("a key is one scalar of 4 words")
        return k

    def scalar_inv(self, scalars, out=None):
        """1 / m_i mod N of every scalar (n, 4) -- any value below 2^256 -- as canonical words (n, 4); 0 where m_i = 0 mod N."""
        s = _host(scalars, 4)
        out = _out(out, len(s), 4)
        self._ck(self._lib.fourq_scalar_inv_batch(self._ctx, _ptr(s), _ptr(out), len(s)))
        return out

    def set_scinv_group(self, k):
        """TEST HOOK (fourq_ctx_set_scinv_group; needs FOURQ_DEBUG_ROUTES=1): 1, 8 or 16 elements per inversion chain, 0 = by batch size."""
        self._ck(self._lib.fourq_ctx_set_scinv_group(self._ctx, int(k)))

    def scalar_inv_dev(self, scalars, out, n):
        self._ck(self._lib.fourq_scalar_inv_batch_dev(self._ctx, _ptr(scalars), _ptr(out), n))

    def oprf_blind(self, msgs, blinds, lens=None, dst=b"", out=None, status=None):
        """encode([r_i]G(msg_i)), G = hash_to_curve(mode "ro") under `dst`: ((n, 32) uint8, status).  status: 0 ok,
        _lib.OPRF_BLIND_ZERO where r_i = 0 mod N (the row is zero then)."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        r = _host(blinds, 4)
        m, stride, lens, msg_len = self._msgs(msgs, lens, len(r))
        out, status = _out(out, len(r), 32, np.uint8), _out(status, len(r), None, np.uint8)
        self._ck(self._lib.fourq_oprf_blind_batch(self._ctx, buf, dst_len, _ptr(m) if stride else None, stride, _ptr(lens), msg_len, _ptr(r), _ptr(out), _ptr(status), len(r)))
        return out, status

    def oprf_blind_dev(self, msgs, stride, lens, msg_len, blinds, out32, status, n, dst=b""):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_oprf_blind_batch_dev(self._ctx, buf, dst_len, _ptr(msgs), stride, _ptr(lens), msg_len, _ptr(blinds), _ptr(out32), _ptr(status), n))

    def oprf_evaluate(self, key, blinded32, out=None, status=None):
        """encode(DH_endo(key, decode(B_i))) with ONE key (4 words) for the batch: ((n, 32) uint8, status) -- dh_bytes with the key on
        every row, status as dh_bytes."""
        k, b = self._key(key), _host(blinded32, 32, np.uint8)
        out, status = _out(out, len(b), 32, np.uint8), _out(status, len(b), None, np.uint8)
        self._ck(self._lib.fourq_oprf_evaluate_batch(self._ctx, _ptr(k), _ptr(b), _ptr(out), _ptr(status), len(b)))
        return out, status

    def oprf_evaluate_dev(self, key_host, blinded32, out32, status, n):
        self._ck(self._lib.fourq_oprf_evaluate_batch_dev(self._ctx, _ptr(self._key(key_host)), _ptr(blinded32), _ptr(out32), _ptr(status), n))

    def oprf_finalize(self, msgs, blinds, evaluated32, lens=None, dst=b"", out=None, status=None):
        """The PRF output of every row: SHA-512(E || msg || "Finalize" || dst || len(dst)) with E = encode([1 / r_i]decode(Z_i)):
        ((n, 64) uint8, status).  status: 0 ok, 16 + decode status, _lib.OPRF_BLIND_ZERO."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        r, z = _host(blinds, 4), _host(evaluated32, 32, np.uint8)
        if len(r) != len(z):
            raise ValueError("blinds and evaluated elements differ in length")
        m, stride, lens, msg_len = self._msgs(msgs, lens, len(r))
        out, status = _out(out, len(r), 64, np.uint8), _out(status, len(r), None, np.uint8)
        self._ck(self._lib.fourq_oprf_finalize_batch(self._ctx, buf, dst_len, _ptr(m) if stride else None, stride, _ptr(lens), msg_len, _ptr(r), _ptr(z), _ptr(out), _ptr(status),
                                                     len(r)))
        return out, status

    def oprf_finalize_dev(self, msgs, stride, lens, msg_len, blinds, evaluated32, out64, status, n, dst=b""):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_oprf_finalize_batch_dev(self._ctx, buf, dst_len, _ptr(msgs), stride, _ptr(lens), msg_len, _ptr(blinds), _ptr(evaluated32), _ptr(out64),
                                                         _ptr(status), n))

    def oprf_eval(self, key, msgs, lens=None, dst=b"", out=None, status=None):
        """The key holder's own evaluation, equal to oprf_finalize(oprf_blind, oprf_evaluate) for every blind: ((n, 64) uint8, status).
        status: 0 ok, _lib.DH_NEUTRAL where key = 0 mod N."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        k = self._key(key)
        m, stride, lens, msg_len = self._msgs(msgs, lens)
        out, status = _out(out, len(m), 64, np.uint8), _out(status, len(m), None, np.uint8)
        self._ck(self._lib.fourq_oprf_eval_batch(self._ctx, _ptr(k), buf, dst_len, _ptr(m) if stride else None, stride, _ptr(lens), msg_len, _ptr(out), _ptr(status), len(m)))
        return out, status

    def oprf_eval_dev(self, key_host, msgs, stride, lens, msg_len, out64, status, n, dst=b""):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_oprf_eval_batch_dev(self._ctx, _ptr(self._key(key_host)), buf, dst_len, _ptr(msgs), stride, _ptr(lens), msg_len, _ptr(out64), _ptr(status), n))

    # ---- oblivious PRF: proofs (fourq_dleq_*: one batched DLEQ proof per group of rows, include/fourq_amd.h) -------------------------
    @staticmethod
    def _pk32(pk32):
        pk = np.ascontiguousarray(np.frombuffer(bytes(pk32), dtype=np.uint8) if isinstance(pk32, (bytes, bytearray)) else pk32, dtype=np.uint8).ravel()
        if pk.size != 32:
            raise ValueError("a public key is 32 bytes")
        return pk

    def _dleq_rows(self, blinded32, evaluated32, group_size):
        b, z = _host(blinded32, 32, np.uint8), _host(evaluated32, 32, np.uint8)
        if len(b) != len(z):
            raise ValueError("blinded and evaluated elements differ in length")
        groups, group_size = self._groups(len(b), max(len(b), 1) if group_size is None else group_size)      # None: one group covers everything
        return b, z, groups, group_size

    def dleq_reserve(self, groups, group_size):
        """Size the context's buffers for `dleq_*_dev` calls of up to groups x group_size rows (fourq_dleq_reserve; reserve() is not
        enough for them): such calls then only enqueue and, with the comb staged, can be captured."""
        self._ck(self._lib.fourq_dleq_reserve(self._ctx, int(groups), int(group_size)))

    def dleq_public_key(self, key):
        """pk32 = encode(DH_endo(key, G)) as (32,) uint8: oprf_evaluate of the generator's encoding."""
        from . import codec
        from .constants import Gx, Gy
        out, status = self.oprf_evaluate(key, self.encode(codec.pack_points([(Gx, Gy)], 2)))
        if status[0]:
            raise ValueError("the key is 0 mod N: it has no public key (status %d)" % int(status[0]))
        return out[0].copy()

    def dleq_composites(self, pk32, blinded32, evaluated32, group_size=None, dst=b"", out=None, status=None):
        """The verifier's composites per group: ((groups, 32) M32, (groups, 32) Z32, status).  group_size None = one group.
        `out`: a pair of arrays."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        pk = self._pk32(pk32)
        b, z, groups, group_size = self._dleq_rows(blinded32, evaluated32, group_size)
        m32, z32 = (None, None) if out is None else out
        m32, z32, status = _out(m32, groups, 32, np.uint8), _out(z32, groups, 32, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_dleq_composites(self._ctx, buf, dst_len, _ptr(pk), _ptr(b), _ptr(z), _ptr(m32), _ptr(z32), _ptr(status), groups, group_size))
        return m32, z32, status

    def dleq_prove(self, key, blinded32, evaluated32, nonces, group_size=None, dst=b"", comb=None, out=None, status=None):
        """One proof c || s per group that evaluated = oprf_evaluate(key, blinded): ((groups, 64) uint8, status).  nonces: (groups, 4)
        words, uniformly random and never reused.  status: 0, BYTES_DECODE_BASE + DECODE_*, DH_NEUTRAL (key = 0 mod N), DLEQ_NONCE_ZERO."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        k, r = self._key(key), _host(nonces, 4)
        b, z, groups, group_size = self._dleq_rows(blinded32, evaluated32, group_size)
        if len(r) != groups:
            raise ValueError("one nonce per group")
        out, status = _out(out, groups, 64, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_dleq_prove(self._ctx, _ptr(k), _ptr(self._comb_arg(comb)), buf, dst_len, _ptr(b), _ptr(z), _ptr(r), _ptr(out), _ptr(status), groups, group_size))
        return out, status

    def dleq_verify(self, pk32, blinded32, evaluated32, proofs64, group_size=None, dst=b"", comb=None, ok=None, status=None):
        """(ok, status) per group: ok[g] = 1 iff proofs64[g] proves the group's rows under pk32.  status says why a 0 is a 0: 0 = the proof
        does not hold, SIG_S_RANGE = c or s >= N, BYTES_DECODE_BASE + DECODE_* = a row or the key does not decode."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        pk, p = self._pk32(pk32), _host(proofs64, 64, np.uint8)
        b, z, groups, group_size = self._dleq_rows(blinded32, evaluated32, group_size)
        if len(p) != groups:
            raise ValueError("one proof per group")
        ok, status = _out(ok, groups, None, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_dleq_verify(self._ctx, _ptr(pk), _ptr(self._comb_arg(comb)), buf, dst_len, _ptr(b), _ptr(z), _ptr(p), _ptr(ok), _ptr(status), groups, group_size))
        return ok, status

    def dleq_composites_dev(self, pk32_host, blinded32, evaluated32, m32, z32, status, groups, group_size, dst=b""):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_dleq_composites_dev(self._ctx, buf, dst_len, _ptr(self._pk32(pk32_host)), _ptr(blinded32), _ptr(evaluated32), _ptr(m32), _ptr(z32), _ptr(status),
                                                     groups, group_size))

    def dleq_prove_dev(self, key_host, blinded32, evaluated32, nonces, proof64, status, groups, group_size, dst=b"", comb_host=None):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_dleq_prove_dev(self._ctx, _ptr(self._key(key_host)), _ptr(self._comb_arg(comb_host)), buf, dst_len, _ptr(blinded32), _ptr(evaluated32), _ptr(nonces),
                                                _ptr(proof64), _ptr(status), groups, group_size))

    def dleq_verify_dev(self, pk32_host, blinded32, evaluated32, proof64, ok, status, groups, group_size, dst=b"", comb_host=None):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_dleq_verify_dev(self._ctx, _ptr(self._pk32(pk32_host)), _ptr(self._comb_arg(comb_host)), buf, dst_len, _ptr(blinded32), _ptr(evaluated32),
                                                 _ptr(proof64), _ptr(ok), _ptr(status), groups, group_size))

    # ---- verifiable random function (fourq_vrf_*, fourq_vrf_verify_keyed*; the construction: include/fourq_amd.h): one row per
    # (key, alpha), keys the signature scheme's; a proof is gamma32 || c || s, 96 bytes; beta is 64 bytes ------------------------------------
    def vrf_reserve(self, n):
        """Size the context's buffers for `vrf_*_dev` calls of at most n rows (fourq_vrf_reserve; reserve() is not enough for them):
        such calls then only enqueue, with the comb staged."""
        self._ck(self._lib.fourq_vrf_reserve(self._ctx, int(n)))

    def vrf_prove(self, sk32, pk32, alphas, lens=None, dst=b"", comb=None, out=None):
        """Proofs (n, 96) uint8 of the rows of `alphas` under the key pairs (sk32[i], pk32[i]).  Deterministic: the nonce is hashed from
        the secret key and the input.  pk32 is an input; it is not checked against sk32."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        sk, pk = _host(sk32, 32, np.uint8), _host(pk32, 32, np.uint8)
        if len(sk) != len(pk):
            raise ValueError("the secret and public key arrays differ in length")
        m, stride, lens, msg_len = self._msgs(alphas, lens, len(sk))
        out = _out(out, len(sk), 96, np.uint8)
        self._ck(self._lib.fourq_vrf_prove(self._ctx, _ptr(sk), _ptr(pk), _ptr(self._comb_arg(comb)), buf, dst_len, _ptr(m) if stride else None, stride, _ptr(lens), msg_len,
                                           _ptr(out), len(sk)))
        return out

    def vrf_prove_dev(self, sk32, pk32, alphas, stride, lens, msg_len, proof96, n, dst=b"", comb_host=None):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_vrf_prove_dev(self._ctx, _ptr(sk32), _ptr(pk32), _ptr(self._comb_arg(comb_host)), buf, dst_len, _ptr(alphas), stride, _ptr(lens), msg_len,
                                               _ptr(proof96), n))

    def vrf_verify(self, pk32, alphas, proofs96, lens=None, dst=b"", comb=None, beta=None, ok=None, status=None):
        """(beta, ok, status) per row: ok[i] = 1 iff proofs96[i] proves alphas[i] under pk32[i]; beta[i], (64,) uint8, is the VRF's output
        then and all zero otherwise.  status says why a 0 is a 0: 0 = the proof does not hold, BYTES_DECODE_BASE + DECODE_* = the key or
        Gamma does not decode, SIG_S_RANGE = c or s >= N, VRF_GAMMA_NEUTRAL = [392]Gamma is the neutral point."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        pk, p = _host(pk32, 32, np.uint8), _host(proofs96, 96, np.uint8)
        if len(pk) != len(p):
            raise ValueError("the key and proof arrays differ in length")
        m, stride, lens, msg_len = self._msgs(alphas, lens, len(pk))
        beta, ok, status = _out(beta, len(pk), 64, np.uint8), _out(ok, len(pk), None, np.uint8), _out(status, len(pk), None, np.uint8)
        self._ck(self._lib.fourq_vrf_verify(self._ctx, _ptr(pk), _ptr(self._comb_arg(comb)), buf, dst_len, _ptr(m) if stride else None, stride, _ptr(lens), msg_len,
                                            _ptr(p), _ptr(beta), _ptr(ok), _ptr(status), len(pk)))
        return beta, ok, status

    def vrf_verify_dev(self, pk32, alphas, stride, lens, msg_len, proof96, beta64, ok, status, n, dst=b"", comb_host=None):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_vrf_verify_dev(self._ctx, _ptr(pk32), _ptr(self._comb_arg(comb_host)), buf, dst_len, _ptr(alphas), stride, _ptr(lens), msg_len,
                                                _ptr(proof96), _ptr(beta64), _ptr(ok), _ptr(status), n))

    def vrf_verify_keyed(self, ids, alphas, proofs96, lens=None, dst=b"", comb=None, beta=None, ok=None, status=None):
        """vrf_verify() with pk32[i] = the registered key ids[i] (keyset_set): (beta, ok, status).  status as vrf_verify's, or the key's
        own status; an index outside the set is an error."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        i, p = np.ascontiguousarray(ids, dtype=np.uint32).ravel(), _host(proofs96, 96, np.uint8)
        if len(i) != len(p):
            raise ValueError("the index and proof arrays differ in length")
        m, stride, lens, msg_len = self._msgs(alphas, lens, len(i))
        beta, ok, status = _out(beta, len(i), 64, np.uint8), _out(ok, len(i), None, np.uint8), _out(status, len(i), None, np.uint8)
        self._ck(self._lib.fourq_vrf_verify_keyed(self._ctx, _ptr(i), _ptr(self._comb_arg(comb)), buf, dst_len, _ptr(m) if stride else None, stride, _ptr(lens), msg_len,
                                                   _ptr(p), _ptr(beta), _ptr(ok), _ptr(status), len(i)))
        return beta, ok, status

    def vrf_verify_keyed_dev(self, ids, alphas, stride, lens, msg_len, proof96, beta64, ok, status, n, dst=b"", comb_host=None):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_vrf_verify_keyed_dev(self._ctx, _ptr(ids), _ptr(self._comb_arg(comb_host)), buf, dst_len, _ptr(alphas), stride, _ptr(lens), msg_len,
                                                       _ptr(proof96), _ptr(beta64), _ptr(ok), _ptr(status), n))

    def vrf_proof_to_hash(self, proofs96, dst=b"", beta=None, status=None):
        """(beta, status) per row from the proof alone (c and s are not looked at): what vrf_verify returns for a proof it accepts.
        status: 0, BYTES_DECODE_BASE + DECODE_*, VRF_GAMMA_NEUTRAL; beta[i] is all zero unless it is 0."""
        buf, dst_len, _ = self._h2c(dst, "ro")
        p = _host(proofs96, 96, np.uint8)
        beta, status = _out(beta, len(p), 64, np.uint8), _out(status, len(p), None, np.uint8)
        self._ck(self._lib.fourq_vrf_proof_to_hash(self._ctx, buf, dst_len, _ptr(p), _ptr(beta), _ptr(status), len(p)))
        return beta, status

    def vrf_proof_to_hash_dev(self, proof96, beta64, status, n, dst=b""):
        buf, dst_len, _ = self._h2c(dst, "ro")
        self._ck(self._lib.fourq_vrf_proof_to_hash_dev(self._ctx, buf, dst_len, _ptr(proof96), _ptr(beta64), _ptr(status), n))

    # ---- threshold sharing (fourq_shamir_*; include/fourq_amd.h, "threshold sharing"): Shamir shares modulo N, Feldman commitments and
    # their check, Lagrange coefficients at 0, combination of scalars and of points.  ids are uint32, never 0.  Party-major: item (i, r) of
    # an array with one item per (party, row) is [i][r].  MultiEngine does not shard these calls ---------------------------------------
    @staticmethod
    def _ids(ids):
        return np.ascontiguousarray(ids, dtype=np.uint32).ravel()

    @staticmethod
    def _poly(coeffs):
        a = np.ascontiguousarray(coeffs, dtype=np.uint64)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("coefficients are (n, t, 4) words: row r's t coefficients together")
        return a

    def shamir_reserve(self, rows, t):
        """Size the context's buffers for `shamir_*_dev` calls of up to rows x t items (fourq_shamir_reserve; reserve() is not enough for
        them): such calls then only enqueue and, with the comb staged, can be captured."""
        self._ck(self._lib.fourq_shamir_reserve(self._ctx, int(rows), int(t)))

    def shamir_shares(self, coeffs, ids, out=None, status=None):
        """shares[p][r] = sum_j coeffs[r][j] ids[p]^j mod N: ((m, n, 4) words party-major, status (m,)).  coeffs: (n, t, 4) words, any
        values below 2^256, coeffs[r][0] the secret.  status[p]: SHAMIR_ID_ZERO where ids[p] == 0 (block p is zero)."""
        a, x = self._poly(coeffs), self._ids(ids)
        n, t, m = a.shape[0], a.shape[1], len(x)
        out, status = _out(None if out is None else out.reshape(m * n, 4), m * n, 4), _out(status, m, None, np.uint8)
        self._ck(self._lib.fourq_shamir_shares(self._ctx, _ptr(a), _ptr(x), _ptr(out), _ptr(status), n, t, m))
        return out.reshape(m, n, 4), status

    def shamir_commitments(self, coeffs, comb=None):
        """The Feldman commitments encode([coeffs[r][j]]G) as (n, t, 32) uint8: the comb over the n x t coefficients, then encode.
        comb: the generator's table, None = the staged one.  No new C entry: comb_mul and encode composed."""
        a = self._poly(coeffs)
        n, t = a.shape[0], a.shape[1]
        affine, st = np.empty((n * t, 8), dtype=np.uint64), np.empty(n * t, dtype=np.uint8)
        self._ck(self._lib.fourq_comb_mul_batch(self._ctx, _ptr(a), _ptr(self._comb_arg(comb)), _ptr(affine), _ptr(st), n * t))
        out = self.encode(affine)
        out[st == _lib.DH_NEUTRAL] = np.array([1] + [0] * 31, dtype=np.uint8)       # the comb reports [0]G by its status and a zero row: 01 00 .. 00 is its encoding
        return out.reshape(n, t, 32)

    def shamir_lagrange(self, ids, out=None, status=None):
        """lambda[set][i] = prod_(j != i) x_j / (x_j - x_i) mod N for ids (sets, t): ((sets, t, 4) words, status (sets,)).  status:
        SHAMIR_ID_ZERO, SHAMIR_ID_REPEATED (the set's rows are all zero then), 0."""
        x = np.ascontiguousarray(ids, dtype=np.uint32)
        if x.ndim != 2:
            raise ValueError("ids are (sets, t)")
        sets, t = x.shape
        out, status = _out(None if out is None else out.reshape(sets * t, 4), sets * t, 4), _out(status, sets, None, np.uint8)
        self._ck(self._lib.fourq_shamir_lagrange(self._ctx, _ptr(x), _ptr(out), _ptr(status), sets, t))
        return out.reshape(sets, t, 4), status

    def shamir_combine(self, ids, shares, out=None):
        """out[r] = sum_i lambda_i shares[i][r] mod N for ONE set of t ids: ((n, 4) words, status).  shares: (t, n, 4) party-major, any
        values below 2^256.  status: one int, shamir_lagrange's codes; non-zero: every row is zero."""
        x, s = self._ids(ids), np.ascontiguousarray(shares, dtype=np.uint64)
        if s.ndim != 3 or s.shape[0] != len(x) or s.shape[2] != 4:
            raise ValueError("shares are (t, n, 4) words, one block per id")
        t, n = s.shape[0], s.shape[1]
        out, status = _out(out, n, 4), np.zeros(1, dtype=np.uint8)
        self._ck(self._lib.fourq_shamir_combine(self._ctx, _ptr(x), _ptr(s), _ptr(out), _ptr(status), n, t))
        return out, int(status[0])

    def shamir_combine_points(self, ids, points32, out=None, status=None):
        """out32[r] = encode(sum_i [lambda_i]decode(points32[i][r])) for ONE set of t ids: ((n, 32) uint8, status (n,)), byte for byte
        msm_bytes over lambda tiled and the points transposed.  points32: (t, n, 32) party-major -- server i's replies are block i."""
        x, p = self._ids(ids), np.ascontiguousarray(points32, dtype=np.uint8)
        if p.ndim != 3 or p.shape[0] != len(x) or p.shape[2] != 32:
            raise ValueError("points are (t, n, 32) bytes, one block per id")
        t, n = p.shape[0], p.shape[1]
        out, status = _out(out, n, 32, np.uint8), _out(status, n, None, np.uint8)
        self._ck(self._lib.fourq_shamir_combine_points(self._ctx, _ptr(x), _ptr(p), _ptr(out), _ptr(status), n, t))
        return out, status

    @staticmethod
    def _commits(commits32, ids):
        c, x = np.ascontiguousarray(commits32, dtype=np.uint8), np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        if c.ndim != 3 or c.shape[0] != len(x) or c.shape[2] != 32:
            raise ValueError("commitments are (groups, t, 32) bytes, with one id per group")
        return c, x

    def shamir_public_shares(self, commits32, ids, out=None, status=None):
        """out32[g] = encode(sum_j [ids[g]^j]decode(commits32[g][j])), party ids[g]'s verification share: ((groups, 32) uint8, status).
        status: msm_bytes's per group, or SHAMIR_ID_ZERO (first; the row is zero)."""
        c, x = self._commits(commits32, ids)
        groups, t = c.shape[0], c.shape[1]
        out, status = _out(out, groups, 32, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_shamir_public_shares(self._ctx, _ptr(c), _ptr(x), _ptr(out), _ptr(status), groups, t))
        return out, status

    def shamir_verify(self, commits32, ids, shares, comb=None, ok=None, status=None):
        """(ok, status) per group: ok[g] = 1 iff shares[g] (4 words) is the value at ids[g] of the polynomial behind commits32[g].
        status: shamir_public_shares's, else SIG_S_RANGE where shares[g] >= N."""
        c, x = self._commits(commits32, ids)
        s = _host(shares, 4)
        groups, t = c.shape[0], c.shape[1]
        if len(s) != groups:
            raise ValueError("one share per group")
        ok, status = _out(ok, groups, None, np.uint8), _out(status, groups, None, np.uint8)
        self._ck(self._lib.fourq_shamir_verify(self._ctx, _ptr(self._comb_arg(comb)), _ptr(c), _ptr(x), _ptr(s), _ptr(ok), _ptr(status), groups, t))
        return ok, status

    def shamir_shares_dev(self, coeffs, ids, shares, status, n, t, m):
        self._ck(self._lib.fourq_shamir_shares_dev(self._ctx, _ptr(coeffs), _ptr(ids), _ptr(shares), _ptr(status), n, t, m))

    def shamir_lagrange_dev(self, ids, lam, status, sets, t):
        self._ck(self._lib.fourq_shamir_lagrange_dev(self._ctx, _ptr(ids), _ptr(lam), _ptr(status), sets, t))

    def shamir_combine_dev(self, ids, shares, out, status, n, t):
        self._ck(self._lib.fourq_shamir_combine_dev(self._ctx, _ptr(ids), _ptr(shares), _ptr(out), _ptr(status), n, t))

    def shamir_combine_points_dev(self, ids, points32, out32, status, n, t):
        self._ck(self._lib.fourq_shamir_combine_points_dev(self._ctx, _ptr(ids), _ptr(points32), _ptr(out32), _ptr(status), n, t))

    def shamir_public_shares_dev(self, commits32, ids, out32, status, groups, t):
        self._ck(self._lib.fourq_shamir_public_shares_dev(self._ctx, _ptr(commits32), _ptr(ids), _ptr(out32), _ptr(status), groups, t))

    def shamir_verify_dev(self, commits32, ids, shares, ok, status, groups, t, comb_host=None):
        self._ck(self._lib.fourq_shamir_verify_dev(self._ctx, _ptr(self._comb_arg(comb_host)), _ptr(commits32), _ptr(ids), _ptr(shares), _ptr(ok), _ptr(status), groups, t))

    def dh_exchange_dev(self, a_scalars, b_scalars, base_affine_host, table392_host, out_affine, status, n):
        base = _host(base_affine_host, None).ravel()
        t = None if table392_host is None else _host(table392_host, None).ravel()
        self._ck(self._lib.fourq_dh_exchange_batch_dev(self._ctx, _ptr(a_scalars), _ptr(b_scalars), _ptr(base), _ptr(t), _ptr(out_affine), _ptr(status), n))

    # ---- fixed-base comb (1024-point table; affine outputs only) -----------------------------------
    def comb_table(self, p_r1):
        """Comb table (_lib.COMB_WORDS words) of the order-N point `p_r1` (fourq_comb_table)."""
        p = _host(p_r1, None).ravel()
        if p.size != 20:
            raise ValueError("an R1 point is 20 words")
        out = np.empty(_lib.COMB_WORDS, dtype=np.uint64)
        self._ck(self._lib.fourq_comb_table(self._ctx, _ptr(p), _ptr(out)))
        return out

    def comb_mul(self, scalars, comb, out=None, status=None):
        """Affine [m_i]B for the comb's base B: ((n, 8) words, status) -- equals R1toAffine(MUL_endo(m_i, B))."""
        s = _host(scalars, 4)
        t = _host(comb, None).ravel()
        if t.size != _lib.COMB_WORDS:
            raise ValueError("a comb table is %d words" % _lib.COMB_WORDS)
        out, status = _out(out, len(s), 8), _out(status, len(s), None, np.uint8)
        self._ck(self._lib.fourq_comb_mul_batch(self._ctx, _ptr(s), _ptr(t), _ptr(out), _ptr(status), len(s)))
        return out, status

    def comb_stage(self, comb):
        """Upload a comb table once (fourq_comb_stage); comb_mul_dev(..., comb_host=None, ...) then uses it with no per-call
        work on the table."""
        t = _host(comb, None).ravel()
        if t.size != _lib.COMB_WORDS:
            raise ValueError("a comb table is %d words" % _lib.COMB_WORDS)
        self._ck(self._lib.fourq_comb_stage(self._ctx, _ptr(t)))

    def comb_mul_dev(self, scalars, comb_host, out_affine, status, n):
        """`comb_host`: the table (compared with the staged copy on every call) or None = the table staged by comb_stage()."""
        t = None
        if comb_host is not None:
            t = _host(comb_host, None).ravel()
            if t.size != _lib.COMB_WORDS:
                raise ValueError("a comb table is %d words" % _lib.COMB_WORDS)
        self._ck(self._lib.fourq_comb_mul_batch_dev(self._ctx, _ptr(scalars), _ptr(t), _ptr(out_affine), _ptr(status), n))

    # ---- point compression (32-byte wire format) -------------------------------------------------
    def encode(self, points_affine, out=None):
        """(n, 8) affine words -> (n, 32) uint8 encodings (curve4q.py:41-46)."""
        p = _host(points_affine, 8)
        out = _out(out, len(p), 32, np.uint8)
        self._ck(self._lib.fourq_encode_batch(self._ctx, _ptr(p), _ptr(out), len(p)))
        return out

    def decode(self, encodings, out=None, status=None):
        """(n, 32) uint8 -> ((n, 8) affine words, (n,) status) (curve4q.py:49-96; status = _lib.DECODE_*)."""
        b = _host(encodings, 32, np.uint8)
        out, status = _out(out, len(b), 8), _out(status, len(b), None, np.uint8)
        self._ck(self._lib.fourq_decode_batch(self._ctx, _ptr(b), _ptr(out), _ptr(status), len(b)))
        return out, status

    def dh_bytes(self, scalars, public_keys32, kind="endo", table=None, out=None, status=None):
        """The protocol step of draft-ladd-cfrg-4q section "Diffie-Hellman": decode each 32-byte public key, DH_<kind> with
        the scalar, encode the shared point -- one call, intermediates stay on the GPU (fourq_dh_*_bytes_batch).
        Returns ((n, 32) uint8, status): 0 ok, 1/2 as DH_*, 16 + decode status."""
        s, k = _host(scalars, 4), _host(public_keys32, 32, np.uint8)
        if len(s) != len(k):
            raise ValueError("scalars and keys differ in length")
        t = None if table is None else _host(table, None).ravel()
        if t is not None and t.size != 128:
            raise ValueError("a table is 128 words")
        out, status = _out(out, len(s), 32, np.uint8), _out(status, len(s), None, np.uint8)
        fn = self._lib.fourq_dh_endo_bytes_batch if kind == "endo" else self._lib.fourq_dh_windowed_bytes_batch
        self._ck(fn(self._ctx, _ptr(s), _ptr(k), _ptr(t), _ptr(out), _ptr(status), len(s)))
        return out, status

    def dh_bytes_dev(self, scalars, keys32, table_host, out32, status, n, kind="endo"):
        t = None if table_host is None else _host(table_host, None).ravel()
        fn = self._lib.fourq_dh_endo_bytes_batch_dev if kind == "endo" else self._lib.fourq_dh_windowed_bytes_batch_dev
        self._ck(fn(self._ctx, _ptr(scalars), _ptr(keys32), _ptr(t), _ptr(out32), _ptr(status), n))

    def encode_dev(self, points_affine, out32, n):
        self._ck(self._lib.fourq_encode_batch_dev(self._ctx, _ptr(points_affine), _ptr(out32), n))

    def decode_dev(self, in32, out_affine, status, n):
        self._ck(self._lib.fourq_decode_batch_dev(self._ctx, _ptr(in32), _ptr(out_affine), _ptr(status), n))

    # ---- device-pointer flavour (async on the engine's stream) ---------------------------------
    def mul_endo_dev(self, scalars, points_r1, out_r1, n):
        self._ck(self._lib.fourq_mul_endo_batch_dev(self._ctx, _ptr(scalars), _ptr(points_r1), _ptr(out_r1), n))

    def mul_windowed_dev(self, scalars, points_r1, out_r1, n):
        self._ck(self._lib.fourq_mul_windowed_batch_dev(self._ctx, _ptr(scalars), _ptr(points_r1), _ptr(out_r1), n))

    def mul_endo_fixed_dev(self, scalars, table_host, out_r1, n):
        t = _host(table_host, None).ravel()
        self._ck(self._lib.fourq_mul_endo_fixed_batch_dev(self._ctx, _ptr(scalars), _ptr(t), _ptr(out_r1), n))

    def mul_windowed_fixed_dev(self, scalars, table_host, out_r1, n):
        t = _host(table_host, None).ravel()
        self._ck(self._lib.fourq_mul_windowed_fixed_batch_dev(self._ctx, _ptr(scalars), _ptr(t), _ptr(out_r1), n))

    def mul_endo_mixed_dev(self, scalars, points_r1, flags, table_host, out_r1, n):
        t = _host(table_host, None).ravel()
        self._ck(self._lib.fourq_mul_endo_mixed_batch_dev(self._ctx, _ptr(scalars), _ptr(points_r1), _ptr(flags), _ptr(t), _ptr(out_r1), n))

    def dh_endo_dev(self, scalars, points_affine, table_host, out_affine, status, n):
        t = None if table_host is None else _host(table_host, None).ravel()
        self._ck(self._lib.fourq_dh_endo_batch_dev(self._ctx, _ptr(scalars), _ptr(points_affine), _ptr(t), _ptr(out_affine), _ptr(status), n))

    def dh_windowed_dev(self, scalars, points_affine, table_host, out_affine, status, n):
        t = None if table_host is None else _host(table_host, None).ravel()
        self._ck(self._lib.fourq_dh_windowed_batch_dev(self._ctx, _ptr(scalars), _ptr(points_affine), _ptr(t), _ptr(out_affine), _ptr(status), n))

    # ---- primitives ----------------------------------------------------------------------------
    def prim(self, op, inputs):
        """Run primitive `op` (name in _lib.PRIM or its int) over rows of `inputs`; returns (n, out_words)."""
        code = PRIM[op] if isinstance(op, str) else int(op)
        iw, ow = ctypes.c_size_t(), ctypes.c_size_t()
        self._ck(self._lib.fourq_prim_words(code, ctypes.byref(iw), ctypes.byref(ow)))
        x = _host(inputs, iw.value)
        out = np.zeros((len(x), ow.value), dtype=np.uint64)
        self._ck(self._lib.fourq_prim_batch(self._ctx, code, _ptr(x), _ptr(out), len(x)))
        return out


_default = None
_default_lock = threading.Lock()


def default_engine():
    """Process-wide engine on device LOCAL_RANK (or 0).  Raises FourQError when no MI355X is usable."""
    global _default
    if _default is None:
        with _default_lock:                    # first calls from several threads at once: one context, not one each
            if _default is None:
                _default = Engine()
    return _default


__all__ = ["Engine", "default_engine", "FourQError"]
