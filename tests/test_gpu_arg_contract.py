"""The argument contract of every per-element host-array entry point and its _dev twin (include/fourq_amd.h), from one table: which
pointers are required, which may be NULL (`table`, `comb`, `lens`, and `msgs` when stride == 0), what n == 0 and n > FOURQ_MAX_BATCH do,
that nothing is staged before the arguments are accepted, and that the _dev forms refuse an array pointer that is not 16-byte aligned.
One fresh context, n <= 3.  Every refused call returns before it touches the device; the accepted ones run with valid pointers.
The grouped sums (fourq_msm_*) take (groups, group_size) instead of n: tests/test_gpu_msm.py pins their rules."""
import ctypes

import numpy as np
import pytest

from fourq_amd import _lib

pytestmark = pytest.mark.gpu

N, STRIDE, DST = 3, 16, b"contract"
PATTERN = 0xA5

# An argument of a call, in the order of the prototype.  Per-element arrays: ("in" | "out", bytes per element), and "in8" / "out8" for the
# byte arrays (flags, ok, status) the _dev forms take at any alignment.  HOST pointers in both flavours: ("host", bytes) is required
# (a fixed-base table, the exchange's base point, a key, a DST), ("table",) and ("comb",) may be NULL.  ("msgs",) stands for the four
# message arguments msgs, stride, lens, msg_len.  ("size", v) and ("int", v) are passed as they are; n is appended.
S32, P160, P64, B32, B64, ST, TABLE, COMB, MSGS = ("in", 32), ("in", 160), ("in", 64), ("in", 32), ("in", 64), ("out8", 1), ("table",), ("comb",), ("msgs",)
DSTARGS = [("host", len(DST)), ("size", len(DST))]
ROWS = {
    "fourq_mul_endo": [S32, P160, ("out", 160)],
    "fourq_mul_windowed": [S32, P160, ("out", 160)],
    "fourq_mul_endo_affine": [S32, P64, ("out", 64)],
    "fourq_mul_windowed_affine": [S32, P64, ("out", 64)],
    "fourq_mul_endo_bytes": [S32, B32, ("out", 32), ST],
    "fourq_mul_windowed_bytes": [S32, B32, ("out", 32), ST],
    "fourq_mul_endo_fixed": [S32, ("host", 1024), ("out", 160)],
    "fourq_mul_windowed_fixed": [S32, ("host", 1024), ("out", 160)],
    "fourq_mul_endo_mixed": [S32, P160, ("in8", 1), ("host", 1024), ("out", 160)],
    "fourq_dh_endo": [S32, P64, TABLE, ("out", 64), ST],
    "fourq_dh_windowed": [S32, P64, TABLE, ("out", 64), ST],
    "fourq_dh_endo_bytes": [S32, B32, TABLE, ("out", 32), ST],
    "fourq_dh_windowed_bytes": [S32, B32, TABLE, ("out", 32), ST],
    "fourq_dh_exchange": [S32, S32, ("host", 64), TABLE, ("out", 64), ST],
    "fourq_dh_exchange_comb": [S32, S32, COMB, ("out", 64), ST],
    "fourq_encode": [P64, ("out", 32)],
    "fourq_decode": [B32, ("out", 64), ST],
    "fourq_comb_mul": [S32, COMB, ("out", 64), ST],
    "fourq_double_mul_affine": [S32, COMB, S32, P64, ("out", 64)],
    "fourq_double_mul_bytes": [S32, COMB, S32, B32, ("out", 32), ST],
    "fourq_verify_bytes": [S32, COMB, S32, B32, B32, ("out8", 1), ST],
    "fourq_sha512": [MSGS, ("out", 64)],
    "fourq_sig_keygen": [B32, COMB, ("out", 32)],
    "fourq_sig_sign": [B32, B32, COMB, MSGS, ("out", 64)],
    "fourq_sig_verify": [B32, COMB, MSGS, B64, ("out8", 1), ST],
    "fourq_hash_to_field": DSTARGS + [("int", _lib.H2C_RO), MSGS, ("out", 64)],
    "fourq_map_to_curve": [S32, ("out", 64)],
    "fourq_hash_to_curve": DSTARGS + [("int", _lib.H2C_RO), MSGS, ("out", 32)],
    "fourq_hash_to_curve_affine": DSTARGS + [("int", _lib.H2C_NU), MSGS, ("out", 64)],
    "fourq_oprf_blind": DSTARGS + [MSGS, S32, ("out", 32), ST],
    "fourq_oprf_evaluate": [("host", 32), B32, ("out", 32), ST],
    "fourq_oprf_finalize": DSTARGS + [MSGS, S32, B32, ("out", 64), ST],
    "fourq_oprf_eval": [("host", 32)] + DSTARGS + [MSGS, ("out", 64), ST],
    "fourq_scalar_inv": [S32, ("out", 32)],
}
CALLS = [(name, flavour) for name in ROWS for flavour in ("host", "dev")]


@pytest.fixture(scope="module")
def fresh():
    from fourq_amd import Engine
    with Engine(0) as e:
        yield e


class Buffers:
    """One buffer per argument of a row, N elements and 16 spare bytes each: numpy for host pointers, torch for device arrays.  Inputs
    hold seeded bytes (any bytes are a valid input to these calls: an encoding that does not decode is a status, not an error), lengths at
    most STRIDE, outputs PATTERN."""
    def __init__(self, spec, flavour):
        import torch
        self.spec, self.dev = spec, flavour == "dev"
        rng = np.random.default_rng(20)
        self.keep, self.addr, self.outs = [], {}, []

        def place(key, host, on_device, out=False):
            if on_device:
                t = torch.from_numpy(host).to(torch.device("cuda", 0))
                assert t.data_ptr() % 16 == 0
                self.keep.append(t)
                self.addr[key] = t.data_ptr()
            else:
                self.keep.append(host)
                self.addr[key] = host.ctypes.data
            if out:
                self.outs.append(self.keep[-1])
        for i, arg in enumerate(spec):
            kind = arg[0]
            if kind in ("in", "in8"):
                place(i, rng.integers(0, 256, size=N * arg[1] + 16, dtype=np.uint8), self.dev)
            elif kind in ("out", "out8"):
                place(i, np.full(N * arg[1] + 16, PATTERN, dtype=np.uint8), self.dev, out=True)
            elif kind == "host":
                place(i, np.frombuffer(DST, dtype=np.uint8).copy() if arg[1] == len(DST) else rng.integers(0, 256, size=arg[1], dtype=np.uint8), False)
            elif kind == "table":
                place(i, rng.integers(0, 256, size=1024, dtype=np.uint8), False)
            elif kind == "comb":
                place(i, rng.integers(0, 256, size=_lib.COMB_WORDS * 8, dtype=np.uint8), False)
            elif kind == "msgs":
                place((i, "msgs"), rng.integers(0, 256, size=N * STRIDE + 16, dtype=np.uint8), self.dev)
                place((i, "lens"), np.array([5, 0, STRIDE] + [0] * 4, dtype=np.uint32).view(np.uint8), self.dev)

    def args(self, n, null=None, shift=None, no_message=None):
        """The call's arguments behind ctx.  null / shift: the key of the pointer passed as NULL / 8 bytes further on; no_message: the
        index of a ("msgs",) entry given as msgs = NULL, stride = 0, lens = NULL, msg_len = 0."""
        ptr = lambda key: None if key == null else ctypes.c_void_p(self.addr[key] + (8 if key == shift else 0))
        out = []
        for i, arg in enumerate(self.spec):
            if arg[0] in ("size", "int"):
                out.append(arg[1])
            elif arg[0] == "msgs":
                out += [None, 0, None, 0] if i == no_message else [ptr((i, "msgs")), STRIDE, ptr((i, "lens")), STRIDE]
            else:
                out.append(ptr(i))
        return out + [n]

    def outputs_untouched(self):
        return all((o.cpu().numpy() if self.dev else o).tolist() == [PATTERN] * len(o) for o in self.outs)


def keys_of(spec, kinds):
    out = []
    for i, arg in enumerate(spec):
        if arg[0] == "msgs":
            out += [(i, sub) for sub in ("msgs", "lens") if sub in kinds]
        elif arg[0] in kinds:
            out.append(i)
    return out


def test_the_table_names_every_per_element_batch_call():
    listed = {name + tail for name in ROWS for tail in ("_batch", "_batch_dev")}
    declared = {n for n in _lib.PROTOTYPES if n.endswith(("_batch", "_batch_dev")) and not n.startswith("fourq_msm_")} - {"fourq_prim_batch"}
    assert listed == declared, sorted(listed ^ declared)
    for name, spec in ROWS.items():         # the table and the prototypes agree on the number of arguments
        assert 1 + sum(4 if a[0] == "msgs" else 1 for a in spec) + 1 == len(_lib.PROTOTYPES[name + "_batch"][1]) == len(_lib.PROTOTYPES[name + "_batch_dev"][1]), name


def test_n_zero_stages_nothing(fresh):
    """First on the fresh context: fourq_comb_mul_batch with a table and n == 0 is FOURQ_OK and stages nothing, so the same call with
    comb == NULL ("the staged table") and n == 1 still finds none."""
    lib = _lib.load()
    b = Buffers(ROWS["fourq_comb_mul"], "host")
    assert lib.fourq_comb_mul_batch(fresh._ctx, *b.args(1, null=1)) == _lib.ERR_INVALID        # nothing was staged before this test either
    assert lib.fourq_comb_mul_batch(fresh._ctx, *b.args(0)) == _lib.OK
    assert lib.fourq_comb_mul_batch(fresh._ctx, *b.args(1, null=1)) == _lib.ERR_INVALID
    assert b.outputs_untouched()


@pytest.mark.parametrize("name,flavour", CALLS, ids=["%s-%s" % c for c in CALLS])
def test_argument_contract(fresh, name, flavour):
    lib = _lib.load()
    spec = ROWS[name]
    fn = getattr(lib, name + ("_batch" if flavour == "host" else "_batch_dev"))
    b = Buffers(spec, flavour)
    call = lambda n, **how: fn(fresh._ctx, *b.args(n, **how))
    # refused, before anything is touched: a required pointer that is NULL, a batch above the limit, a misaligned device array
    for key in keys_of(spec, ("in", "in8", "out", "out8", "host", "msgs")):
        assert call(N, null=key) == _lib.ERR_INVALID, key
    assert call(_lib.MAX_BATCH + 1) == _lib.ERR_INVALID
    if flavour == "dev":
        for key in keys_of(spec, ("in", "out", "msgs", "lens")):
            assert call(N, shift=key) == _lib.ERR_INVALID, key
    # n == 0: accepted, nothing written
    assert call(0) == _lib.OK
    fresh.sync()
    assert b.outputs_untouched()
    # accepted: every argument given (this also stages the row's comb), then each pointer that may be NULL left out in turn
    assert call(N) == _lib.OK
    for key in keys_of(spec, ("table", "comb", "lens")):
        assert call(N, null=key) == _lib.OK, key
    for i in keys_of(spec, ("msgs",)):
        if isinstance(i, tuple) and i[1] == "msgs":
            assert call(N, no_message=i[0]) == _lib.OK, i
    fresh.sync()
    assert not b.outputs_untouched()
