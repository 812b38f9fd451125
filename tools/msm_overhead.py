#!/usr/bin/env python3
"""What the fold and the per-group lowering of a grouped sum cost on top of the ladder (GPU box).

    python tools/msm_overhead.py  > profiles/msm_overhead.txt

msm_dev (affine in, affine out) against mul_affine_dev (MUL_endo, affine I/O) over the same n = 2^16 elements, device-resident, in this
process, alternating, for (groups, group_size) = (1024, 64), (256, 256), (1, 65536) and both selection modes.  Each figure: median of
--steps event-timed calls after --warmup warm-up calls; the shader clock under load is printed beside them.  The two calls share the
ladder; they differ in what follows it: mul_affine_dev lowers n rows (one inversion per element at this size), msm_dev runs 1, 2 or 3
fold passes and lowers `groups` rows.  A ratio below 1 therefore says that the fold costs less than the n - groups inversions it replaces.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=16)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
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


n = 1 << args.log2n
k, t = seeded_scalars(7400, n), seeded_scalars(7401, n)
P, _ = eng.comb_mul(t, comb)
kd, Pd = to_dev(k), to_dev(P)
out = torch.empty((n, 8), dtype=torch.int64, device=dev)
eng.reserve(n)
shapes = [(n >> 6, 64), (n >> 8, 256), (1, n)]
sums = {s: torch.empty((s[0], 8), dtype=torch.int64, device=dev) for s in shapes}
fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % v

print("grouped-sum overhead: msm_dev against mul_affine_dev, n = 2^%d device-resident, median (min .. max) of %d event-timed calls after %d warm-up calls, alternating" % (
    args.log2n, args.steps, args.warmup))
print("lanes %d   build %s" % (eng.lanes, eng.build_id))
results = {}
for ct in (False, True):
    eng.ct_select = ct
    for _ in range(40):
        eng.mul_affine_dev(kd, Pd, out, n)
    clock = eng.diag_clock(4000)
    torch.cuda.synchronize()
    print("[%s] clock under load %.0f MHz" % ("constant-time selection" if ct else "default selection", clock["mhz"]))
    for groups, size in shapes:
        msm, mul = timed_pair(lambda: eng.msm_dev(kd, Pd, sums[groups, size], groups, size), lambda: eng.mul_affine_dev(kd, Pd, out, n))
        results[ct, groups, size] = sums[groups, size].cpu().numpy().copy()
        print("  groups %5d x %5d   msm_dev %s   mul_affine_dev %s   ratio %.3f   difference %+.1f us" % (
            groups, size, fmt(msm), fmt(mul), msm[0] / mul[0], (msm[0] - mul[0]) * 1e3))
for groups, size in shapes:
    assert np.array_equal(results[False, groups, size], results[True, groups, size]), "the selection modes disagree"
# the three shapes are one computation grouped differently: the finer sums add up to the coarser ones (checked through the library's own call)
one = np.ascontiguousarray(np.tile(np.array([1, 0, 0, 0], dtype=np.uint64), (n >> 6, 1)))
again = eng.msm(one, results[False, n >> 6, 64].view(np.uint64), n >> 6)
assert np.array_equal(again, results[False, 1, n].view(np.uint64)), "the sum of the 64-element sums is not the whole sum"
print("both selection modes gave identical sums; the 64-element sums add up to the whole sum")
eng.close()
