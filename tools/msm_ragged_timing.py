#!/usr/bin/env python3
"""The ragged grouped sums against what a caller does without them, and against the equal-length call where the lengths are equal (GPU box).

    python tools/msm_ragged_timing.py  > profiles/msm_ragged_timing.txt

msm_ragged_dev (affine in, affine out) over device-resident arrays, in this process, alternating with its baseline, default selection mode:
  padded   msm_dev over the same groups padded to the longest length with scalar 0 (and some valid point), for 1024 groups of 1 .. 127 rows,
           for 1023 groups of 8 rows and one of 8192, and for 65536 groups of 0 .. 2 rows;
  equal    msm_dev itself at 1024 x 64, 256 x 256 and 1 x 65536, the shapes of profiles/msm_overhead.txt: what the descriptors cost.
Each figure: median (min .. max) of --steps event-timed calls after --warmup warm-up calls; every pair is timed --rounds times, so the
baseline has several medians of the SAME call: their relative spread (max / min - 1) is what a difference has to exceed to mean anything.
The shader clock under load is printed beside each shape, and the two calls' outputs are compared byte for byte.  Last: the host time of
msm_shape (fourq_raggedsum_shape_set: validate, plan, upload, synchronise) for the second and third shape, median of --steps calls.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import seeded_scalars  # noqa: E402
from fourq_amd import Engine, codec, constants  # noqa: E402

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
eng = Engine(0, stream=stream.cuda_stream)
g1 = codec.pack_point((constants.Gx, constants.Gy, (1, 0), constants.Gx, constants.Gy))
comb = eng.comb_table(g1)
rng = np.random.default_rng(8200)
RAGGED = [("1024 groups of 1 .. 127 rows", rng.integers(1, 128, size=1024)),
          ("1023 groups of 8 rows and one of 8192", np.array([8] * 511 + [8192] + [8] * 512)),
          ("65536 groups of 0 .. 2 rows", rng.integers(0, 3, size=65536))]
EQUAL = [(1024, 64), (256, 256), (1, 65536)]


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def timed_pair(f, g):
    """Medians (min .. max) of the event-timed calls of f and of g, alternating, in ms."""
    for _ in range(args.warmup):
        f()
        g()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(args.steps):
        for fn, into in ((f, ms[0]), (g, ms[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            into.append(a.elapsed_time(b))
    return tuple((statistics.median(m), min(m), max(m)) for m in ms)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)


def compare(name, lengths, groups, size, kd, Pd, k_base, P_base):
    """msm_ragged_dev on (kd, Pd) with the shape `lengths` against msm_dev on (k_base, P_base) as groups x size; returns the summary row"""
    n = int(np.sum(lengths))
    eng.msm_shape(offsets_of(lengths))
    eng.msm_shape_reserve()
    want = torch.empty((groups, 8), dtype=torch.int64, device=dev)
    got = torch.empty((groups, 8), dtype=torch.int64, device=dev)
    for _ in range(20):
        eng.msm_dev(k_base, P_base, want, groups, size)
    clock = eng.diag_clock(4000)
    torch.cuda.synchronize()
    print("%s: %d rows; baseline msm_dev %d x %d = %d rows   clock under load %.0f MHz" % (name, n, groups, size, groups * size, clock["mhz"]))
    ragged, base = [], []
    for r in range(args.rounds):
        a, b = timed_pair(lambda: eng.msm_ragged_dev(kd, Pd, got), lambda: eng.msm_dev(k_base, P_base, want, groups, size))
        assert torch.equal(got, want), "the two calls disagree at " + name
        ragged.append(a[0])
        base.append(b[0])
        print("  round %d   msm_ragged_dev %s   msm_dev %s   ratio %.3f" % (r, fmt(a), fmt(b), a[0] / b[0]))
    spread = max(base) / min(base) - 1
    row = (name, statistics.median(ragged), statistics.median(base), spread)
    print("  median of medians: msm_ragged_dev %.4f ms, msm_dev %.4f ms, ratio %.3f; msm_dev's spread (max / min - 1) %.1f %%" % (row[1], row[2], row[1] / row[2], 100 * spread))
    return row


n_pool = 1 << 17
k, t = seeded_scalars(7400, n_pool), seeded_scalars(7401, n_pool)
P, _ = eng.comb_mul(t, comb)
kd, Pd = to_dev(k), to_dev(P)
fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % v

print("ragged grouped sums: msm_ragged_dev against msm_dev, device-resident, default selection, median (min .. max) of %d event-timed calls "
      "after %d warm-up calls, alternating, %d rounds per shape" % (args.steps, args.warmup, args.rounds))
print("lanes %d   build %s" % (eng.lanes, eng.build_id))
summary = []
print("against the padded call: every group padded to the longest with scalar 0")
for name, lengths in RAGGED:
    lengths = np.asarray(lengths, dtype=np.int64)
    groups, size, n = len(lengths), int(lengths.max()), int(lengths.sum())
    offs = offsets_of(lengths).astype(np.int64)
    dest = to_dev(np.repeat(np.arange(groups) * size - offs[:-1], lengths) + np.arange(n))
    k_pad = torch.zeros((groups * size, 4), dtype=torch.int64, device=dev)
    P_pad = Pd[:1].repeat(groups * size, 1)
    k_pad[dest] = kd[:n]
    P_pad[dest] = Pd[:n]
    summary.append(compare(name, lengths, groups, size, kd, Pd, k_pad, P_pad))
    del k_pad, P_pad
print("against the equal-length call at equal lengths: what the descriptors cost")
for groups, size in EQUAL:
    summary.append(compare("%d x %d" % (groups, size), [size] * groups, groups, size, kd, Pd, kd, Pd))
print("per shape: time as a fraction of the baseline's, and the baseline's own spread")
for name, a, b, spread in summary:
    verdict = "faster" if a < b / (1 + spread) else "slower" if b < a / (1 + spread) else "within the spread"
    print("  %-40s msm_ragged_dev %.4f ms   msm_dev %.4f ms   ratio %.3f   spread %.1f %%   %s" % (name, a, b, a / b, 100 * spread, verdict))
print("msm_shape on the host (validate, plan, upload, synchronise), median (min .. max) of %d calls" % args.steps)
for name, lengths in RAGGED[1:]:
    offs = offsets_of(lengths)
    ms = []
    for _ in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        eng.msm_shape(offs)
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = ms[args.warmup:]
    print("  %-40s %d groups   %.4f ms (%.4f .. %.4f)" % (name, len(lengths), statistics.median(ms), min(ms), max(ms)))
eng.close()
