#!/usr/bin/env python3
"""Timings of the double-scalar route [k]B + [l]P against the two calls a user composed before it existed (GPU box).

    python tools/double_mul_probe.py --ref-lib <libfourq_amd.so of the parent commit>  > profiles/double_mul.txt

T_ref = mul_affine_dev (MUL_endo, affine I/O) + comb_mul_dev, each at n = 2^16 device-resident, measured on the PARENT commit's
library in a child process of this run (FOURQ_AMD_LIB; the child binds only the symbols that library has); T_new = double_mul_dev
(affine out) at the same n on this tree's library.  Each figure: median of --steps event-timed steps after --warmup warm-up steps,
default selection; the shader clock under load is printed beside both so that they can be stated in cycles per element.  Also
printed, not compared with anything: verify_bytes_dev at 2^16, the host-array verify_bytes at 2^20 from pinned arrays, and all
three with constant-time selection.  Without --ref-lib only the new figures are printed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--ref-lib", default="", help="library of the parent commit (built from a checkout of it with python -m fourq_amd.build --out)")
ap.add_argument("--log2n", type=int, default=16)
ap.add_argument("--log2n-host", type=int, default=20)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--role", default="main", choices=["main", "ref"])
args = ap.parse_args()

if args.role == "ref":
    # the parent's library lacks the symbols this tree's binding declares: bind what is there
    import ctypes
    import torch  # noqa: F401  (first, as fourq_amd/_lib.py does: the library must bind the HIP runtime torch brings)
    from fourq_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(have, n)]:
        del _lib.PROTOTYPES[name]

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
eng.comb_stage(comb)


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def timed(fn):
    """Median of the event-timed steps, in ms."""
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


n = 1 << args.log2n
k, l, t = (seeded_scalars(7000 + i, n) for i in range(3))
P, _ = eng.comb_mul(t, comb)
kd, ld, Pd = to_dev(k), to_dev(l), to_dev(P)
out = torch.empty((n, 8), dtype=torch.int64, device=dev)
out2 = torch.empty((n, 8), dtype=torch.int64, device=dev)
st = torch.empty(n, dtype=torch.uint8, device=dev)

if args.role == "ref":
    mul = timed(lambda: eng.mul_affine_dev(ld, Pd, out, n))
    cmb = timed(lambda: eng.comb_mul_dev(kd, None, out2, st, n))
    both = timed(lambda: (eng.mul_affine_dev(ld, Pd, out, n), eng.comb_mul_dev(kd, None, out2, st, n)))
    clock = clock_under(lambda: eng.mul_affine_dev(ld, Pd, out, n))
    print(json.dumps({"build_id": eng.build_id, "mul_affine_dev_ms": mul, "comb_mul_dev_ms": cmb, "both_in_one_bracket_ms": both, "clock": clock}))
    sys.exit(0)

ref = None
if args.ref_lib:
    env = dict(os.environ, FOURQ_AMD_LIB=os.path.abspath(args.ref_lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "ref", "--log2n", str(args.log2n), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    proc = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    if proc.returncode != 0:
        sys.exit("the reference run failed:\n" + proc.stdout + proc.stderr)
    ref = json.loads(proc.stdout.strip().splitlines()[-1])

print("double-scalar multiplication probe: n = 2^%d device-resident, median (min .. max) of %d event-timed steps after %d warm-up steps" % (args.log2n, args.steps, args.warmup))
print("lanes %d" % eng.lanes)
fmt = lambda v: "%.4f ms (%.4f .. %.4f)" % v
want = eng.double_mul(k, l, P)
keys, expect = eng.encode(P), eng.encode(want)
keysd, expectd = to_dev(keys), to_dev(expect)
okd = torch.empty(n, dtype=torch.uint8, device=dev)
rows = {}
for ct in (False, True):
    eng.ct_select = ct
    mode = "constant-time selection" if ct else "default selection"
    rows[ct] = new = timed(lambda: eng.double_mul_dev(kd, ld, Pd, out, n))
    ver = timed(lambda: eng.verify_bytes_dev(kd, ld, keysd, expectd, okd, st, n))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want) and okd.cpu().numpy().all()
    clock = clock_under(lambda: eng.double_mul_dev(kd, ld, Pd, out, n))
    print("[%s] build %s" % (mode, eng.build_id))
    print("  double_mul_dev (affine out)   %s   %.1f M/s   clock under load %.0f MHz -> %.2f shader cycles of chip time per element" % (
        fmt(new), n / new[0] / 1e3, clock["mhz"], new[0] * 1e3 * clock["mhz"] / n))
    print("  verify_bytes_dev              %s   %.1f M verifications/s" % (fmt(ver), n / ver[0] / 1e3))
    if not ct and ref:
        t_ref = ref["mul_affine_dev_ms"][0] + ref["comb_mul_dev_ms"][0]
        print("  parent build %s (same box, same session, child process): clock under load %.0f MHz" % (ref["build_id"], ref["clock"]["mhz"]))
        print("    mul_affine_dev (endo)       %s" % fmt(tuple(ref["mul_affine_dev_ms"])))
        print("    comb_mul_dev                %s" % fmt(tuple(ref["comb_mul_dev_ms"])))
        print("    both in one event bracket   %s" % fmt(tuple(ref["both_in_one_bracket_ms"])))
        print("    T_ref in shader cycles of chip time per element: %.2f" % (t_ref * 1e3 * ref["clock"]["mhz"] / n))
        print("  T_ref = %.4f ms   T_new = %.4f ms   T_new / T_ref = %.3f   (required: <= 1.05)" % (t_ref, new[0], new[0] / t_ref))
    # host arrays, pinned: 97 bytes in, 2 out per signature
    nh = 1 << args.log2n_host
    reps = -(-nh // n)
    big = [eng.host_array(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:nh]) for a in (k, l, keys, expect)]
    ok_h, st_h = eng.host_empty(nh, np.uint8), eng.host_empty(nh, np.uint8)
    wall = []
    for i in range(2 + 5):
        t0 = time.perf_counter()
        eng.verify_bytes(big[0], big[1], big[2], big[3], ok=ok_h, status=st_h)
        wall.append((time.perf_counter() - t0) * 1e3)
    assert ok_h.all() and not st_h.any()
    w = sorted(wall[2:])
    print("  verify_bytes, 2^%d pinned host arrays   %.3f ms (%.3f .. %.3f, wall clock, 5 calls after 2)   %.1f M verifications/s   %d chunks" % (
        args.log2n_host, w[2], w[0], w[-1], nh / w[2] / 1e3, eng.host_stats()["chunks"]))
    for a in big + [ok_h, st_h]:
        eng.host_free(a)
eng.close()
