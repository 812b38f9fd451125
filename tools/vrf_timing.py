#!/usr/bin/env python3
"""The verifiable random function on the device: verify against the sum of its inner calls, keyed against unkeyed, and prove (GPU box).

    python tools/vrf_timing.py  > profiles/vrf_timing.txt

Everything is device-resident, alpha is 32 bytes, proofs are honest ones (made by vrf_prove_dev in this process), and every figure is taken
in default mode and in constant-time mode at 4 096, 65 536 and 2^20 rows.  Each figure: median (min .. max) of --steps event-timed calls
after --warmup warm-up calls, the calls of one comparison alternating; the shader clock under load is printed beside each shape.

(a) vrf_verify_dev against the sum of its inner calls timed on their own on the same rows: hash_to_curve_dev (of 64-byte rows: pk32 ||
    alpha as the device hashes them), double_mul_bytes_dev ([s]G + [c]Y) and msm_bytes_dev over n groups of two.  Each inner call is
    timed in two halves of the steps; the margin is the sum of the differences of their half-run medians.  What remains of verify beyond
    the sum is the new kernels' share (the cleared Gamma, the challenge and output hashes).
(b) vrf_verify_keyed_dev against vrf_verify_dev on pk32 = keys[ids], ids uniform random, over 1, 256 and 4 096 registered keys; beta, ok
    and status of the two calls are compared byte for byte at every shape.
(c) vrf_prove_dev: rows per second.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--max-log2n", type=int, default=20)
ap.add_argument("--keys", type=int, default=4096)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fourq_amd import Engine, codec, constants  # noqa: E402

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
eng = Engine(0, stream=stream.cuda_stream)
g1 = codec.pack_point((constants.Gx, constants.Gy, (1, 0), constants.Gx, constants.Gy))
comb = eng.comb_table(g1)
eng.comb_stage(comb)
SIZES = [n for n in (1 << 12, 1 << 16, 1 << 20) if n <= 1 << args.max_log2n]
KEYS = [m for m in (1, 256, 4096) if m <= args.keys]
ALPHA = 32
DST = b"FourQ-VRF-V01-timing"


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


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

n_max, m_max = max(SIZES), max(KEYS)
rng = np.random.default_rng(8700)
sks = rng.integers(0, 256, size=(m_max, 32), dtype=np.uint8)
keys = eng.sig_keygen(sks)
alpha = rng.integers(0, 256, size=(n_max, ALPHA), dtype=np.uint8)
d_alpha = to_dev(alpha)
eng.reserve(2 * n_max)
eng.keyset_reserve(n_max)
eng.vrf_reserve(n_max)

print("the VRF on the device: device-resident, alpha of %d bytes, honest proofs, median (min .. max) of %d event-timed calls after %d warm-up calls, "
      "alternating inside a comparison" % (ALPHA, args.steps, args.warmup))
print("lanes %d   build %s" % (eng.lanes, eng.build_id))
for ct in (False, True):
    eng.ct_select = ct
    mode = "constant-time selection" if ct else "default mode"
    for n in SIZES:
        beta_k, beta_u, ok_k, ok_u, st_k, st_u = u8(n, 64), u8(n, 64), u8(n), u8(n), u8(n), u8(n)
        for m in KEYS:
            status = eng.keyset_set(keys[:m])
            assert not status.any()
            ids = rng.integers(0, m, size=n).astype(np.uint32)
            d_ids, d_pk, d_sk, d_proof = to_dev(ids), to_dev(keys[ids]), to_dev(sks[ids]), u8(n, 96)
            prove = lambda: eng.vrf_prove_dev(d_sk, d_pk, d_alpha, ALPHA, None, ALPHA, d_proof, n, dst=DST)
            prove()
            keyed = lambda: eng.vrf_verify_keyed_dev(d_ids, d_alpha, ALPHA, None, ALPHA, d_proof, beta_k, ok_k, st_k, n, dst=DST)
            unkeyed = lambda: eng.vrf_verify_dev(d_pk, d_alpha, ALPHA, None, ALPHA, d_proof, beta_u, ok_u, st_u, n, dst=DST)
            keyed(); unkeyed()
            for _ in range(5):
                unkeyed()
            clock = eng.diag_clock(4000)
            torch.cuda.synchronize()
            assert bool(ok_u.all()) and not bool(st_u.any()), "an honest proof was refused at n %d, m %d, %s" % (n, m, mode)
            assert torch.equal(beta_k, beta_u) and torch.equal(ok_k, ok_u) and torch.equal(st_k, st_u), "keyed and unkeyed disagree at n %d, m %d, %s" % (n, m, mode)
            print("%s   n %d rows   m %d keys   clock under load %.0f MHz" % (mode, n, m, clock["mhz"]))
            first, second = two_halves([keyed, unkeyed])
            k, u = (stat(a + b) for a, b in zip(first, second))
            halves = [statistics.median(first[1]), statistics.median(second[1])]
            print("  (b) vrf_verify_keyed_dev %s   ratio to vrf_verify_dev %.3f" % (fmt(k), k[0] / u[0]))
            print("      vrf_verify_dev       %s   its two half-run medians %.4f and %.4f ms: spread %.1f %%" % (fmt(u), halves[0], halves[1], 100 * (max(halves) / min(halves) - 1)))
            if m != KEYS[-1]:
                continue
            # (a) the inner calls on the same rows: 64-byte rows pk32 || alpha, (s, c) and pk32, n groups of two over (s, h32), (c, h32)
            d_rows = torch.cat([d_pk.view(n, 32), d_alpha[:n].view(n, ALPHA)], dim=1).contiguous()
            h32, out32, st = u8(n, 32), u8(n, 32), u8(n)
            s_rows, c_rows = d_proof.view(n, 96)[:, 64:].contiguous(), d_proof.view(n, 96)[:, 32:64].contiguous()
            pair_sc = torch.stack([s_rows, c_rows], dim=1).contiguous()
            h2c = lambda: eng.hash_to_curve_dev(d_rows, 32 + ALPHA, None, 32 + ALPHA, h32, n, dst=DST)
            h2c()
            torch.cuda.synchronize()
            pair_pt = torch.stack([h32, h32], dim=1).contiguous()
            pair_out, pair_st = u8(n, 32), u8(n)
            double = lambda: eng.double_mul_bytes_dev(s_rows, c_rows, d_pk, out32, st, n)
            msm = lambda: eng.msm_bytes_dev(pair_sc, pair_pt, pair_out, pair_st, n, 2)
            first, second = two_halves([unkeyed, h2c, double, msm])
            whole = stat(first[0] + second[0])
            parts = [stat(a + b) for a, b in zip(first[1:], second[1:])]
            margin = sum(abs(statistics.median(a) - statistics.median(b)) for a, b in zip(first[1:], second[1:]))
            total = sum(p[0] for p in parts)
            print("  (a) vrf_verify_dev       %s" % fmt(whole))
            for name, p in zip(("hash_to_curve_dev   ", "double_mul_bytes_dev", "msm_bytes_dev, n x 2"), parts):
                print("      %s %s" % (name, fmt(p)))
            print("      sum of the inner calls %.4f ms, margin (their half-run medians' differences) %.4f ms; verify - sum = %.4f ms (%.1f %% of verify): %s"
                  % (total, margin, whole[0] - total, 100 * (whole[0] - total) / whole[0],
                     "the new kernels' share" if whole[0] - total > margin else "within the margin"))
            first, second = two_halves([prove])
            p = stat(first[0] + second[0])
            print("  (c) vrf_prove_dev        %s   %.2f M rows / s" % (fmt(p), n / p[0] / 1e3))
            del d_rows, pair_sc, pair_pt
        del beta_k, beta_u
eng.close()
