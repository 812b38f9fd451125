#!/usr/bin/env python3
"""Threshold sharing on the device: what combine_points adds to the grouped sum, the dealing rate, and verify against its inner calls (GPU box).

    python tools/shamir_timing.py  > profiles/shamir_timing.txt

Everything is device-resident.  Each figure: median (min .. max) of --steps event-timed calls after --warmup warm-up calls, the calls of one
comparison alternating inside a round; a comparison is taken in two halves of the steps, and the baseline's two half-run medians give its
spread.  The shader clock under load is printed beside each shape.

(a) shamir_combine_points_dev against msm_bytes_dev on operands ALREADY tiled and transposed (what a caller had to prepare on the host
    before), n x t = 2^16 x 3, 2^14 x 16, 2^10 x 256, in default and in constant-time mode.  The ratio is the price of the Lagrange
    kernels and the filler; shamir_lagrange_dev over the same one set is timed beside them, and the filler's byte traffic (it reads 32
    and writes 64 bytes per element) is printed.
(b) shamir_shares_dev in (party, row) evaluations per second at t = 3, 16, 256 with m = 5 parties and n = 2^16 rows, and beside it the
    same polynomials evaluated with Python integers on the host (Horner's rule, `% N`), which is what a caller did before: timed on the
    first --host-rows rows and all five parties with time.perf_counter, and compared with the device's shares on those rows.
(c) shamir_verify_dev against the sum of its inner calls (msm_bytes_dev over host-made powers, comb_mul_dev, encode_dev) at 2^12 groups
    x t = 16, honest shares, in both modes.
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--host-rows", type=int, default=256)
ap.add_argument("--scale", type=int, default=0, help="shift every row count down by this many bits (a rehearsal)")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fourq_amd import Engine, codec, constants  # noqa: E402

N = constants.N
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
eng = Engine(0, stream=stream.cuda_stream)
g1 = codec.pack_point((constants.Gx, constants.Gy, (1, 0), constants.Gx, constants.Gy))
eng.comb_stage(eng.comb_table(g1))
COMBINE = [(n >> args.scale, t) for n, t in ((1 << 16, 3), (1 << 14, 16), (1 << 10, 256))]
DEAL_N, DEAL_M, DEAL_T = (1 << 16) >> args.scale, 5, (3, 16, 256)
VERIFY = ((1 << 12) >> args.scale, 16)
rng = np.random.default_rng(8800)
pyrng = random.Random(8801)


def to_dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(dev)


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


def two_halves(calls):
    for _ in range(max(args.warmup, 1)):
        for fn in calls:
            fn()
    torch.cuda.synchronize()
    half = max(args.steps // 2, 1)
    return timed(calls, half), timed(calls, max(args.steps - half, 1))


stat = lambda m: (statistics.median(m), min(m), max(m))
fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % v
u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
scalars = lambda count: rng.integers(0, 1 << 62, size=(count, 4), dtype=np.uint64)      # below 2^254, above N now and then: any value is a scalar


def points(count):
    """`count` encodings of points of order N on the device: the comb over random scalars, then encode"""
    affine, st, out = torch.empty((count, 8), dtype=torch.int64, device=dev), u8(count), u8(count, 32)
    eng.comb_mul_dev(to_dev(scalars(count)), None, affine, st, count)
    eng.encode_dev(affine, out, count)
    torch.cuda.synchronize()
    return out


def clock_after(fn):
    for _ in range(5):
        fn()
    mhz = eng.diag_clock(4000)["mhz"]
    torch.cuda.synchronize()
    return mhz


print("threshold sharing on the device: device-resident, median (min .. max) of %d event-timed calls after %d warm-up calls, alternating inside a comparison"
      % (args.steps, args.warmup))
print("lanes %d   build %s" % (eng.lanes, eng.build_id))
eng.reserve(max(n * t for n, t in COMBINE + [VERIFY]))
for n, t in COMBINE + [VERIFY]:
    eng.shamir_reserve(n, t)

# ---- (a) combine_points against the grouped sum on prepared operands -------------------------------------------------------------------
for ct in (False, True):
    eng.ct_select = ct
    mode = "constant-time selection" if ct else "default mode"
    for n, t in COMBINE:
        ids = np.array(pyrng.sample(range(1, 1 << 32), t), dtype=np.uint32)
        d_ids, d_pts = to_dev(ids), points(n * t)                                     # party-major t x n
        lam, st = eng.shamir_lagrange(ids.reshape(1, t))
        assert not st.any()
        tiled = to_dev(np.tile(lam[0], (n, 1)))
        transposed = d_pts.view(t, n, 32).transpose(0, 1).contiguous().view(n * t, 32)
        out_c, st_c, out_m, st_m = u8(n, 32), u8(n), u8(n, 32), u8(n)
        combine = lambda: eng.shamir_combine_points_dev(d_ids, d_pts, out_c, st_c, n, t)
        msm = lambda: eng.msm_bytes_dev(tiled, transposed, out_m, st_m, n, t)
        d_lam, d_lst = torch.empty((t, 4), dtype=torch.int64, device=dev), u8(1)
        lagrange = lambda: eng.shamir_lagrange_dev(d_ids, d_lam, d_lst, 1, t)
        combine(); msm(); lagrange()
        clock = clock_after(msm)
        assert torch.equal(out_c, out_m) and torch.equal(st_c, st_m) and not bool(st_c.any()), "combine_points and msm_bytes disagree at %d x %d, %s" % (n, t, mode)
        first, second = two_halves([combine, msm, lagrange])
        c, m, l = (stat(a + b) for a, b in zip(first, second))
        halves = [statistics.median(first[1]), statistics.median(second[1])]
        spread = max(halves) / min(halves) - 1
        print("%s   (a) n %d rows x t %d   clock under load %.0f MHz" % (mode, n, t, clock))
        print("  shamir_combine_points_dev %s   ratio to msm_bytes_dev %.3f" % (fmt(c), c[0] / m[0]))
        print("  msm_bytes_dev, prepared   %s   its two half-run medians %.4f and %.4f ms: spread %.1f %%" % (fmt(m), halves[0], halves[1], 100 * spread))
        print("  shamir_lagrange_dev, 1 set %s   t lanes, one inversion chain each: a latency that does not depend on n" % fmt(l))
        print("  combine_points - msm = %.4f ms; less the Lagrange kernels %.4f ms for the filler (%.1f MB read and written) and the merge"
              % (c[0] - m[0], c[0] - m[0] - l[0], 96 * n * t / 1e6))
        del d_pts, transposed, tiled
eng.ct_select = False

# ---- (b) dealing: device against Python integers on the host ----------------------------------------------------------------------------
for t in DEAL_T:
    n, m = DEAL_N, DEAL_M
    coeffs = scalars(n * t)
    ids = np.array([1, 2, 7, 1000003, (1 << 32) - 1], dtype=np.uint32)
    d_coeffs, d_ids, d_shares, d_st = to_dev(coeffs), to_dev(ids), torch.empty((m * n, 4), dtype=torch.int64, device=dev), u8(m)
    deal = lambda: eng.shamir_shares_dev(d_coeffs, d_ids, d_shares, d_st, n, t, m)
    deal()
    clock = clock_after(deal)
    first, second = two_halves([deal])
    d = stat(first[0] + second[0])
    halves = [statistics.median(first[0]), statistics.median(second[0])]
    rows = min(args.host_rows, n)
    polys = [codec.unpack_scalars(coeffs[r * t:(r + 1) * t]) for r in range(rows)]
    xs = [int(x) for x in ids]
    begin = time.perf_counter()
    want = []
    for x in xs:
        for poly in polys:
            acc = 0
            for a in reversed(poly):
                acc = (acc * x + a) % N
            want.append(acc)
    host_s = time.perf_counter() - begin
    got = d_shares.cpu().numpy().view(np.uint64).reshape(m, n, 4)[:, :rows]
    assert codec.unpack_scalars(np.ascontiguousarray(got)) == want and not bool(d_st.any()), "the device's shares differ from Python's at t %d" % t
    print("(b) shamir_shares_dev   t %d, m %d parties x n %d rows   clock under load %.0f MHz" % (t, m, n, clock))
    print("  device %s   half-run medians %.4f and %.4f ms   %.1f M evaluations / s (%.2f G Horner steps / s)"
          % (fmt(d), halves[0], halves[1], m * n / d[0] / 1e3, m * n * t / d[0] / 1e6))
    print("  Python integers on the host, %d rows x %d parties: %.4f s, %.4f M evaluations / s: the device is %.0f times as fast"
          % (rows, m, host_s, m * rows / host_s / 1e6, (m * n / d[0] * 1e3) / (m * rows / host_s)))
    del d_coeffs, d_shares

# ---- (c) verify against the sum of its inner calls ------------------------------------------------------------------------------------------
groups, t = VERIFY
coeffs = np.ascontiguousarray(codec.pack_scalars([int(v) % (N - 1) + 1 for v in codec.unpack_scalars(scalars(groups * t))]))
d_coeffs, d_seven = to_dev(coeffs), to_dev(np.full(groups, 7, dtype=np.uint32))
affine, st_comb, d_commits = torch.empty((groups * t, 8), dtype=torch.int64, device=dev), u8(groups * t), u8(groups * t, 32)
eng.comb_mul_dev(d_coeffs, None, affine, st_comb, groups * t)
eng.encode_dev(affine, d_commits, groups * t)
d_shares, d_st = torch.empty((groups, 4), dtype=torch.int64, device=dev), u8(1)
eng.shamir_shares_dev(d_coeffs, d_seven, d_shares, d_st, groups, t, 1)
powers = to_dev(np.tile(codec.pack_scalars([pow(7, j, N) for j in range(t)]), (groups, 1)))
for ct in (False, True):
    eng.ct_select = ct
    mode = "constant-time selection" if ct else "default mode"
    ok, st, pub, st_pub, aff, st_c, g32 = u8(groups), u8(groups), u8(groups, 32), u8(groups), torch.empty((groups, 8), dtype=torch.int64, device=dev), u8(groups), u8(groups, 32)
    verify = lambda: eng.shamir_verify_dev(d_commits, d_seven, d_shares, ok, st, groups, t)
    msm = lambda: eng.msm_bytes_dev(powers, d_commits, pub, st_pub, groups, t)
    comb = lambda: eng.comb_mul_dev(d_shares, None, aff, st_c, groups)
    encode = lambda: eng.encode_dev(aff, g32, groups)
    verify(); msm(); comb(); encode()
    clock = clock_after(verify)
    assert bool(ok.all()) and not bool(st.any()) and torch.equal(pub, g32), "an honest share was refused, %s" % mode
    first, second = two_halves([verify, msm, comb, encode])
    whole = stat(first[0] + second[0])
    parts = [stat(a + b) for a, b in zip(first[1:], second[1:])]
    margin = sum(abs(statistics.median(a) - statistics.median(b)) for a, b in zip(first[1:], second[1:]))
    total = sum(p[0] for p in parts)
    print("%s   (c) %d groups x t %d   clock under load %.0f MHz" % (mode, groups, t, clock))
    print("  shamir_verify_dev %s" % fmt(whole))
    for name, p in zip(("msm_bytes_dev, host-made powers", "comb_mul_dev                   ", "encode_dev                     "), parts):
        print("      %s %s" % (name, fmt(p)))
    print("      sum of the inner calls %.4f ms, margin (their half-run medians' differences) %.4f ms; verify - sum = %.4f ms (%.1f %% of verify): %s"
          % (total, margin, whole[0] - total, 100 * (whole[0] - total) / whole[0],
             "the powers and compare kernels' share" if whole[0] - total > margin else "within the margin"))
eng.close()
