#!/usr/bin/env python3
"""Fixed-generator commitments against the ladder route over the tiled bases, per shape and route (GPU box).

    python tools/commit_timing.py  > profiles/commit_timing.txt

commit_dev at route 1 (staged) and route 2 (gather) against msm_dev over the bases tiled `groups` times -- the way to the same bytes without
a generator set -- over device-resident arrays, in this process, the three calls alternating.  Default selection mode at (groups x
group_size) 32768 x 2, 1024 x 64, 64 x 1024, 1 x 4096 and 65536 x 1, constant-time mode at 1024 x 64.  Each figure: median (min .. max) of
--steps event-timed calls after --warmup warm-up calls of every call; the shader clock under load is printed beside each shape.  msm_dev
is timed in two halves of the steps, so every shape has two medians of the SAME call: their relative spread (max / min - 1) is what a
difference between the two routes has to exceed to mean anything.  The three outputs are compared byte for byte at every shape.  Then the
time of commit_bases (synchronous, host clock) for 64 and 1 024 bases, and the block the route table in fourq_amd.hip (COMMIT_ROUTES) is
derived from: per shape the faster route, and whether it beats the other by more than that spread.
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
ap.add_argument("--max-log2n", type=int, default=16)
ap.add_argument("--bases", type=int, default=4096)
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
fits = lambda s: s[0] * s[1] <= 1 << args.max_log2n and s[1] <= args.bases
SHAPES = [s for s in ((32768, 2), (1024, 64), (64, 1024), (1, 4096), (65536, 1)) if fits(s)]
CT_SHAPES = [s for s in ((1024, 64),) if fits(s)]


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def timed(calls, steps):
    """Per call the event-timed durations in ms of `steps` rounds, the calls alternating inside a round."""
    ms = [[] for _ in calls]
    for _ in range(steps):
        for fn, into in zip(calls, ms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize()
            into.append(a.elapsed_time(b))
    return ms


stat = lambda m: (statistics.median(m), min(m), max(m))
fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % v

n_max = max(g * s for g, s in SHAPES + CT_SHAPES)
m_max = max(s for _, s in SHAPES + CT_SHAPES)
k = seeded_scalars(7500, n_max)
B, _ = eng.comb_mul(seeded_scalars(7501, m_max), comb)
kd = to_dev(k)
eng.reserve(n_max)

print("commitments through per-base combs against the ladder route: commit_dev(route 1 = staged, 2 = gather) against msm_dev over the tiled bases, "
      "device-resident, median (min .. max) of %d event-timed calls after %d warm-up calls, alternating" % (args.steps, args.warmup))
print("lanes %d   build %s" % (eng.lanes, eng.build_id))
set_times = []
for m in (64, 1024):
    if m <= m_max:
        t0 = time.perf_counter()
        eng.commit_bases(B[:m])
        set_times.append((m, 1e3 * (time.perf_counter() - t0)))
t0 = time.perf_counter()
eng.commit_bases(B)
set_times.append((m_max, 1e3 * (time.perf_counter() - t0)))
for m, ms in set_times:
    print("commit_bases, %4d bases: %.1f ms (one synchronous call, host clock; %.3f ms per base)" % (m, ms, ms / m))

summary = []
for ct, shapes in ((False, SHAPES), (True, CT_SHAPES)):
    eng.ct_select = ct
    for groups, size in shapes:
        n = groups * size
        Pd = to_dev(np.tile(B[:size], (groups, 1)))
        want, got1, got2 = (torch.empty((groups, 8), dtype=torch.int64, device=dev) for _ in range(3))
        eng.commit_reserve(groups, size)
        calls = [lambda: eng.commit_dev(kd, got1, groups, size, 1), lambda: eng.commit_dev(kd, got2, groups, size, 2), lambda: eng.msm_dev(kd, Pd, want, groups, size)]
        for _ in range(max(args.warmup, 1)):
            for fn in calls:
                fn()
        for _ in range(20):
            eng.msm_dev(kd, Pd, want, groups, size)
        clock = eng.diag_clock(4000)
        torch.cuda.synchronize()
        assert torch.equal(got1, want) and torch.equal(got2, want), "the routes disagree at %d x %d" % (groups, size)
        half = max(args.steps // 2, 1)
        first, second = timed(calls, half), timed(calls, max(args.steps - half, 1))
        staged, gather, ladder = (stat(a + b) for a, b in zip(first, second))
        halves = [statistics.median(first[2]), statistics.median(second[2])]
        spread = max(halves) / min(halves) - 1
        assert torch.equal(got1, want) and torch.equal(got2, want), "the routes disagree at %d x %d" % (groups, size)
        mode = "constant-time" if ct else "default"
        print("%s mode, groups %d x %d   clock under load %.0f MHz" % (mode, groups, size, clock["mhz"]))
        print("  commit_dev staged %s   ratio to msm_dev %.3f" % (fmt(staged), staged[0] / ladder[0]))
        print("  commit_dev gather %s   ratio to msm_dev %.3f%s" % (fmt(gather), gather[0] / ladder[0], "   (the route makes no difference in this mode)" if ct else ""))
        print("  msm_dev           %s   its two half-run medians %.4f and %.4f ms: spread %.1f %%" % (fmt(ladder), halves[0], halves[1], 100 * spread))
        summary.append((mode, groups, size, staged[0], gather[0], ladder[0], spread))
        del Pd
print("per shape: the faster route, and whether it beats the other by more than msm_dev's spread")
for mode, groups, size, s, g, m, spread in summary:
    verdict = "staged" if s < g / (1 + spread) else "gather" if g < s / (1 + spread) else "either (within the spread)"
    if mode != "default":
        verdict = "one kernel: two timings of the same launch"
    print("  %-13s groups %6d x %5d   staged %.4f ms (%.3f of msm_dev)   gather %.4f ms (%.3f)   msm_dev %.4f ms   spread %.1f %%   faster: %s"
          % (mode, groups, size, s, s / m, g, g / m, m, 100 * spread, verdict))
eng.close()
