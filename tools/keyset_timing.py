#!/usr/bin/env python3
"""Signature checks over registered keys against the unkeyed route on the same rows, per batch size, key count and id pattern (GPU box).

    python tools/keyset_timing.py  > profiles/keyset_timing.txt

sig_verify_keyed_dev (the generator's comb and key id's comb in one accumulator) against sig_verify_dev with pk32 = keys[ids] (a comb, a
variable-base ladder and the combiner) over device-resident arrays, in this process, the two calls alternating.  Default selection mode
only: constant-time selection runs the unkeyed route on the gathered key bytes.  Shapes: n of 65536 and 2^20 rows, m of 1, 16, 256 and 4096
keys, ids uniform random and sorted.  Messages of 32 bytes, honest keys, signature bytes random with s < N: the work does not depend on
whether a row verifies, and ok and status of the two calls are compared byte for byte at every shape.  Each figure: median (min .. max) of
--steps event-timed calls after --warmup warm-up calls of either call; the shader clock under load is printed beside each shape.  The
unkeyed call is timed in two halves of the steps, so every shape has two medians of the SAME call: their relative spread (max / min - 1)
is what a difference between the routes has to exceed to mean anything.  Then the time of keyset_set (synchronous, host clock) for 64
and 4096 keys, and per shape whether the keyed route is faster by more than that spread.
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
SIZES = [n for n in (1 << 16, 1 << 20) if n <= 1 << args.max_log2n]
KEYS = [m for m in (1, 16, 256, 4096) if m <= args.keys]
MSG = 32


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


stat = lambda m: (statistics.median(m), min(m), max(m))
fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % v

n_max, m_max = max(SIZES), max(KEYS)
rng = np.random.default_rng(7600)
keys = eng.sig_keygen(rng.integers(0, 256, size=(m_max, 32), dtype=np.uint8))
sig = rng.integers(0, 256, size=(n_max, 64), dtype=np.uint8)
sig[:, 62:] = 0                                                     # s < 2^240 < N: no row is refused for its range
d_sig, d_msg = to_dev(sig), to_dev(rng.integers(0, 256, size=(n_max, MSG), dtype=np.uint8))
eng.reserve(n_max)
eng.keyset_reserve(n_max)

print("signature checks over registered keys against the unkeyed route: sig_verify_keyed_dev against sig_verify_dev on pk32 = keys[ids], "
      "device-resident, median (min .. max) of %d event-timed calls after %d warm-up calls, alternating" % (args.steps, args.warmup))
print("lanes %d   build %s   messages of %d bytes" % (eng.lanes, eng.build_id, MSG))
for m in sorted({min(64, m_max), m_max}):
    t0 = time.perf_counter()
    status = eng.keyset_set(keys[:m])
    ms = 1e3 * (time.perf_counter() - t0)
    assert not status.any()
    print("keyset_set, %4d keys: %.1f ms (one synchronous call, host clock; %.3f ms per key)" % (m, ms, ms / m))

summary = []
for n in SIZES:
    ok_k, st_k, ok_u, st_u = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(4))
    for m in KEYS:
        eng.keyset_set(keys[:m])
        for pattern in ("random", "sorted"):
            ids = rng.integers(0, m, size=n).astype(np.uint32)
            if pattern == "sorted":
                ids.sort()
            d_ids, d_pk = to_dev(ids), to_dev(keys[ids])
            calls = [lambda: eng.sig_verify_keyed_dev(d_ids, d_msg, MSG, None, MSG, d_sig, ok_k, st_k, n),
                     lambda: eng.sig_verify_dev(d_pk, d_msg, MSG, None, MSG, d_sig, ok_u, st_u, n)]
            for _ in range(max(args.warmup, 1)):
                for fn in calls:
                    fn()
            for _ in range(5):
                calls[1]()
            clock = eng.diag_clock(4000)
            torch.cuda.synchronize()
            assert torch.equal(ok_k, ok_u) and torch.equal(st_k, st_u), "the routes disagree at n %d, m %d, %s ids" % (n, m, pattern)
            half = max(args.steps // 2, 1)
            first, second = timed(calls, half), timed(calls, max(args.steps - half, 1))
            keyed, unkeyed = (stat(a + b) for a, b in zip(first, second))
            halves = [statistics.median(first[1]), statistics.median(second[1])]
            spread = max(halves) / min(halves) - 1
            assert torch.equal(ok_k, ok_u) and torch.equal(st_k, st_u), "the routes disagree at n %d, m %d, %s ids" % (n, m, pattern)
            print("n %d rows, m %d keys, %s ids   clock under load %.0f MHz" % (n, m, pattern, clock["mhz"]))
            print("  sig_verify_keyed_dev %s   ratio to sig_verify_dev %.3f" % (fmt(keyed), keyed[0] / unkeyed[0]))
            print("  sig_verify_dev       %s   its two half-run medians %.4f and %.4f ms: spread %.1f %%" % (fmt(unkeyed), halves[0], halves[1], 100 * spread))
            summary.append((n, m, pattern, keyed[0], unkeyed[0], spread))
            del d_ids, d_pk
print("per shape: whether the keyed route is faster than the unkeyed one by more than the spread of the unkeyed route's own timings")
for n, m, pattern, k, u, spread in summary:
    verdict = "faster" if k < u / (1 + spread) else "NOT faster beyond the spread"
    print("  n %8d   m %5d   %-6s ids   keyed %.4f ms   unkeyed %.4f ms   ratio %.3f   spread %.1f %%   %s" % (n, m, pattern, k, u, k / u, 100 * spread, verdict))
eng.close()
