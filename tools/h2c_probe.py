#!/usr/bin/env python3
"""Timing of hash to curve on the device against the library's unchanged point multiplication (GPU box).

    python tools/h2c_probe.py  > profiles/h2c.txt

T_h2c = hash_to_curve_dev (RO, 32-byte messages, a 43-byte DST, 32-byte points out) at n = 2^16 device-resident rows; T_mul =
mul_endo_bytes_batch_dev (decode + MUL_endo + encode) at the same n, in the same process on the same box.  Median of --steps event-timed
steps after --warmup, shader clock under load beside each, both table-selection modes (hash to curve has one code path; the ladder has
two).  Expected from instruction counts: T_h2c / T_mul near 0.5.  Requirement: T_h2c / T_mul < 1.0 in the default mode -- a guard against
spills or divergence, not a tuned figure.  The two halves of the call (hash_to_field_dev, map_to_curve_dev on its output) are timed beside
it, and the NU flavour.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=16)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fourq_amd import Engine, codec, constants, h2c  # noqa: E402

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
eng = Engine(0, stream=stream.cuda_stream)
n = 1 << args.log2n
DST = h2c.KAT_DST[:43]


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dev)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def clock_under(fn):
    for _ in range(40):
        fn()
    c = eng.diag_clock(4000)
    torch.cuda.synchronize()
    return c


fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % tuple(v)
print("hash-to-curve probe: n = 2^%d device-resident, median (min .. max) of %d event-timed steps after %d warm-up steps; build %s; lanes %d" % (
    args.log2n, args.steps, args.warmup, eng.build_id, eng.lanes))
msgs = np.random.default_rng(32).integers(0, 256, size=(n, 32), dtype=np.uint8)
md = to_dev(msgs)
out32 = torch.empty((n, 32), dtype=torch.uint8, device=dev)
u = torch.empty((n, 2, 4), dtype=torch.int64, device=dev)
aff = torch.empty((2 * n, 8), dtype=torch.int64, device=dev)
st = torch.empty(n, dtype=torch.uint8, device=dev)
eng.reserve(n)
# the multiplication's inputs: random scalars, and the points the hash just produced (valid encodings of points of order N)
points = eng.hash_to_curve(msgs, dst=DST)
assert points[0].tobytes() == h2c.hash_to_curve(msgs[0].tobytes(), DST)
scalars = to_dev(np.random.default_rng(7).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64))
pd = to_dev(points)
mul_out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
for ct in (False, True):
    eng.ct_select = ct
    mode = "constant-time selection" if ct else "default selection"
    t_h2c = timed(lambda: eng.hash_to_curve_dev(md, 32, None, 32, out32, n, dst=DST, mode="ro"))
    torch.cuda.synchronize()
    assert np.array_equal(out32.cpu().numpy(), points)
    c_h2c = clock_under(lambda: eng.hash_to_curve_dev(md, 32, None, 32, out32, n, dst=DST, mode="ro"))
    t_mul = timed(lambda: eng.mul_bytes_dev(scalars, pd, mul_out, st, n))
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    c_mul = clock_under(lambda: eng.mul_bytes_dev(scalars, pd, mul_out, st, n))
    print("[%s]" % mode)
    print("  hash_to_curve_dev (RO, 32-byte messages, 43-byte DST, bytes out) %s  %.1f M/s  clock under load %.0f MHz" % (fmt(t_h2c), n / t_h2c[0] / 1e3, c_h2c["mhz"]))
    print("  mul_endo_bytes_batch_dev                                         %s  %.1f M/s  clock under load %.0f MHz" % (fmt(t_mul), n / t_mul[0] / 1e3, c_mul["mhz"]))
    print("  T(hash_to_curve_dev) / T(mul_endo_bytes_batch_dev) = %.3f%s" % (t_h2c[0] / t_mul[0], "   (required: < 1.0; expected near 0.5)" if not ct else ""))
eng.ct_select = False
t_f = timed(lambda: eng.hash_to_field_dev(md, 32, None, 32, u, n, dst=DST, mode="ro"))
t_m = timed(lambda: eng.map_to_curve_dev(u, aff, 2 * n))
t_nu = timed(lambda: eng.hash_to_curve_dev(md, 32, None, 32, out32, n, dst=DST, mode="nu"))
print("the halves: hash_to_field_dev (RO: three compressions per row) %s | map_to_curve_dev on its 2^%d elements (map + one inversion each, no x392) %s" % (
    fmt(t_f), args.log2n + 1, fmt(t_m)))
print("hash_to_curve_dev, NU flavour: %s" % fmt(t_nu))
eng.close()
