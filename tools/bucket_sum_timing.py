#!/usr/bin/env python3
"""The bucket route of the grouped sums against the ladder route, per shape and window (GPU box).

    python tools/bucket_sum_timing.py  > profiles/bucket_sum_timing.txt

bucket_sum_dev (affine in, affine out, explicit window) against msm_dev over the same device-resident arrays, in this process, alternating,
default selection mode, for (groups, group_size) = (1, 4096), (1, 65536), (16, 4096), (256, 256) and (1, 2^20) -- and, to place the threshold
between the last two group sizes, (1, 2^18) and (1, 2^19) -- and every window 6..12 whose
work buffer stays below --max-gib.  Each figure: median of --steps event-timed calls after --warmup warm-up calls; the shader clock under
load is printed beside each shape.  msm_dev is timed once per window, so every shape has several medians of the SAME call: their relative
spread (max / min - 1) is the run-to-run spread a difference between two routes has to exceed to mean anything.  The last block is what the
default-window table in fourq_amd.hip (BUCKET_WINDOWS) is derived from: per shape the fastest option, and whether it beats the ladder route
by more than that spread.  The two routes' outputs are compared byte for byte at every (shape, window).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--max-gib", type=float, default=6.0)
ap.add_argument("--max-log2n", type=int, default=20)
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
WINDOWS = range(6, 13)
SHAPES = [s for s in ((1, 4096), (1, 65536), (16, 4096), (256, 256), (1, 1 << 18), (1, 1 << 19), (1, 1 << 20)) if s[0] * s[1] <= 1 << args.max_log2n]


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def work_bytes(groups, size, c):
    """fourq_amd/csrc/bucket_layout.h, Bucket::bytes, to within the status regions' rounding"""
    n, W, B = groups * size, -(-64 // c), 1 << c
    cols = groups * 4 * W
    rows = [size]
    for _ in range(2):
        rows.append(min(rows[-1], min(B - 1, rows[-1]) + rows[-1] // 64))
    chunks = B // 16
    return 394 * n + 97 * n + cols * (4 * B + 8 * (B + 1) + 4 * size + 96 * (rows[1] + rows[2] + chunks + -(-chunks // 64) + 1)) + 500 * groups


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


n_max = max(g * s for g, s in SHAPES)
k, t = seeded_scalars(7400, n_max), seeded_scalars(7401, n_max)
P, _ = eng.comb_mul(t, comb)
kd, Pd = to_dev(k), to_dev(P)
eng.reserve(n_max)
fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % v

print("bucket route against ladder route: bucket_sum_dev(window) against msm_dev, device-resident, default selection, median (min .. max) of %d "
      "event-timed calls after %d warm-up calls, alternating" % (args.steps, args.warmup))
print("lanes %d   build %s" % (eng.lanes, eng.build_id))
summary = []
for groups, size in SHAPES:
    n = groups * size
    want = torch.empty((groups, 8), dtype=torch.int64, device=dev)
    got = torch.empty((groups, 8), dtype=torch.int64, device=dev)
    for _ in range(20):
        eng.msm_dev(kd, Pd, want, groups, size)
    clock = eng.diag_clock(4000)
    torch.cuda.synchronize()
    print("groups %d x %d   clock under load %.0f MHz" % (groups, size, clock["mhz"]))
    ladder, bucket = [], {}
    for c in WINDOWS:
        need = work_bytes(groups, size, c)
        if need > args.max_gib * 2 ** 30:
            print("  window %2d   skipped: the work buffer would take %.1f GiB" % (c, need / 2 ** 30))
            continue
        eng.bucket_sum_reserve(groups, size, c)
        b, m = timed_pair(lambda: eng.bucket_sum_dev(kd, Pd, got, groups, size, c), lambda: eng.msm_dev(kd, Pd, want, groups, size))
        assert torch.equal(got, want), "the routes disagree at %d x %d, window %d" % (groups, size, c)
        ladder.append(m[0])
        bucket[c] = b[0]
        print("  window %2d   bucket_sum_dev %s   msm_dev %s   ratio %.3f   work buffer %.0f MiB" % (c, fmt(b), fmt(m), b[0] / m[0], need / 2 ** 20))
    spread = max(ladder) / min(ladder) - 1
    best = min(bucket, key=bucket.get)
    summary.append((groups, size, statistics.median(ladder), spread, best, bucket[best]))
    print("  msm_dev over its %d timings: median of medians %.4f ms, spread (max / min - 1) %.1f %%" % (len(ladder), statistics.median(ladder), 100 * spread))
print("per shape: the ladder route, its spread, the fastest bucket window, and the fastest option")
for groups, size, m, spread, best, b in summary:
    verdict = "window %d" % best if b < m / (1 + spread) else "the ladder route" if m < b / (1 + spread) else "either (within the spread)"
    print("  groups %5d x %7d   msm_dev %.4f ms   spread %.1f %%   best window %2d: %.4f ms   ratio %.3f   fastest: %s" % (groups, size, m, 100 * spread, best, b, b / m, verdict))
eng.close()
