#!/usr/bin/env python3
"""Timings of the signature layer (SHA-512 and mod-N arithmetic on the device) against what the parent commit offered (GPU box).

    python tools/sig_probe.py --ref-lib <libfourq_amd.so of the parent commit>  > profiles/schnorrq.txt

Verify: T_parent = verify_bytes_dev of the PARENT commit's library at n = 2^16 device-resident with h hashed on the host beforehand,
measured in a child process of this run (FOURQ_AMD_LIB; the child binds only the symbols that library has); T_new = sig_verify_dev on
this tree's library on the same rows; this tree's own verify_bytes_dev beside both.  Median of --steps event-timed steps after --warmup,
shader clock under load beside each.  Requirement (32-byte messages, default selection): T_new / T_parent <= 1.10.
Also: sha512_dev at 2^20 rows of 112 bytes, sig_sign_dev / sig_keygen_dev against the parent's comb_mul_dev + encode_dev, the host-array
sig_verify at 2^20 from pinned arrays next to verify_bytes.  Without --ref-lib only this tree's figures are printed.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--ref-lib", default="")
ap.add_argument("--log2n", type=int, default=16)
ap.add_argument("--log2n-host", type=int, default=20)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--role", default="main", choices=["main", "ref"])
ap.add_argument("--rows", default="", help="(ref role) .npz with s, h, pk, R of the rows to verify")
args = ap.parse_args()

if args.role == "ref":
    import ctypes
    import torch  # noqa: F401  (first, as fourq_amd/_lib.py does)
    from fourq_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(have, n)]:
        del _lib.PROTOTYPES[name]

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
N = constants.N


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
n = 1 << args.log2n

if args.role == "ref":
    rows = np.load(args.rows)
    sd, hd, pkd, Rd = (to_dev(rows[k]) for k in ("s", "h", "pk", "R"))
    ok, st = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    out8, out32 = torch.empty((n, 8), dtype=torch.int64, device=dev), torch.empty((n, 32), dtype=torch.uint8, device=dev)
    res = {"build_id": eng.build_id}
    for ct in (False, True):
        eng.ct_select = ct
        res["verify_bytes_dev_ms_ct%d" % ct] = timed(lambda: eng.verify_bytes_dev(sd, hd, pkd, Rd, ok, st, n))
        torch.cuda.synchronize()
        assert ok.cpu().numpy().all()
        res["clock_ct%d" % ct] = clock_under(lambda: eng.verify_bytes_dev(sd, hd, pkd, Rd, ok, st, n))
        res["comb_encode_dev_ms_ct%d" % ct] = timed(lambda: (eng.comb_mul_dev(sd, None, out8, st, n), eng.encode_dev(out8, out32, n)))
    print(json.dumps(res))
    sys.exit(0)

print("signature probe: n = 2^%d device-resident, median (min .. max) of %d event-timed steps after %d warm-up steps; build %s; lanes %d" % (
    args.log2n, args.steps, args.warmup, eng.build_id, eng.lanes))
sk = np.random.default_rng(1).integers(0, 256, size=(n, 32), dtype=np.uint8)
pk = eng.sig_keygen(sk)
ok = torch.empty(n, dtype=torch.uint8, device=dev)
st = torch.empty(n, dtype=torch.uint8, device=dev)
skd, pkd = to_dev(sk), to_dev(pk)
ref = None
for length in (32, 200, 1000):
    msgs = np.random.default_rng(length).integers(0, 256, size=(n, (length + 15) // 16 * 16), dtype=np.uint8)
    lens = np.full(n, length, dtype=np.uint32)
    sig = eng.sig_sign(sk, pk, msgs, lens)
    md, ld, sigd = to_dev(msgs), to_dev(lens), to_dev(sig)
    stride = msgs.shape[1]
    # the rows as the scalar-level call wants them: h hashed on the host
    h = codec.pack_scalars([int.from_bytes(hashlib.sha512(sig[i, :32].tobytes() + pk[i].tobytes() + msgs[i, :length].tobytes()).digest(), "little") % N for i in range(n)])
    s_words = np.ascontiguousarray(sig[:, 32:]).view("<u8").reshape(n, 4)
    R = np.ascontiguousarray(sig[:, :32])
    sd, hd, Rd = to_dev(s_words), to_dev(h), to_dev(R)
    if length == 32 and args.ref_lib:
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "sig_probe_rows_%d.npz" % os.getpid())
        np.savez(path, s=s_words, h=h, pk=pk, R=R)
        env = dict(os.environ, FOURQ_AMD_LIB=os.path.abspath(args.ref_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--role", "ref", "--rows", path, "--log2n", str(args.log2n), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        proc = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        os.remove(path)
        if proc.returncode != 0:
            sys.exit("the reference run failed:\n" + proc.stdout + proc.stderr)
        ref = json.loads(proc.stdout.strip().splitlines()[-1])
        print("parent build %s (same box, same session, child process)" % ref["build_id"])
    print("messages of %d bytes (row stride %d)" % (length, stride))
    for ct in (False, True):
        eng.ct_select = ct
        mode = "constant-time selection" if ct else "default selection"
        new = timed(lambda: eng.sig_verify_dev(pkd, md, stride, ld, 0, sigd, ok, st, n))
        torch.cuda.synchronize()
        assert ok.cpu().numpy().all() and not st.cpu().numpy().any()
        own = timed(lambda: eng.verify_bytes_dev(sd, hd, pkd, Rd, ok, st, n))
        clock = clock_under(lambda: eng.sig_verify_dev(pkd, md, stride, ld, 0, sigd, ok, st, n))
        print("  [%s] sig_verify_dev %s  %.1f M/s  clock under load %.0f MHz | this tree's verify_bytes_dev %s" % (mode, fmt(new), n / new[0] / 1e3, clock["mhz"], fmt(own)))
        if ref:
            par = ref["verify_bytes_dev_ms_ct%d" % ct]
            note = "   (required: <= 1.10)" if length == 32 and not ct else ""
            print("      parent verify_bytes_dev (32-byte rows' s, h, pk, R) %s  clock %.0f MHz   T(sig_verify_dev) / T_parent(verify_bytes_dev) = %.3f%s" % (
                fmt(par), ref["clock_ct%d" % ct]["mhz"], new[0] / par[0], note))
    if length == 32:
        sig_out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        pk_out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        for ct in (False, True):
            eng.ct_select = ct
            sign = timed(lambda: eng.sig_sign_dev(skd, pkd, md, stride, ld, 0, sig_out, n))
            keyg = timed(lambda: eng.sig_keygen_dev(skd, pk_out, n))
            torch.cuda.synchronize()
            assert np.array_equal(sig_out.cpu().numpy(), sig) and np.array_equal(pk_out.cpu().numpy(), pk)
            line = "  [%s] sig_sign_dev %s   sig_keygen_dev %s" % ("constant-time" if ct else "default", fmt(sign), fmt(keyg))
            if ref:
                line += "   parent comb_mul_dev + encode_dev %s" % fmt(ref["comb_encode_dev_ms_ct%d" % ct])
            print(line)
        eng.ct_select = False
        # host arrays, pinned: pk, sig and a 32-byte message are 128 bytes in per row, 2 out
        nh = 1 << args.log2n_host
        reps = -(-nh // n)
        big = [eng.host_array(np.tile(a, (reps, 1))[:nh]) for a in (pk, msgs[:, :32], sig, s_words, h, R)]
        ok_h, st_h = eng.host_empty(nh, np.uint8), eng.host_empty(nh, np.uint8)
        for name, call in (("sig_verify", lambda: eng.sig_verify(big[0], big[1], big[2], ok=ok_h, status=st_h)),
                           ("verify_bytes", lambda: eng.verify_bytes(big[3], big[4], big[0], big[5], ok=ok_h, status=st_h))):
            wall = []
            for i in range(2 + 5):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            assert ok_h.all() and not st_h.any()
            w = sorted(wall[2:])
            print("  %s, 2^%d pinned host arrays   %.3f ms (%.3f .. %.3f, wall clock, 5 calls after 2)   %.1f M/s   %d chunks" % (
                name, args.log2n_host, w[2], w[0], w[-1], nh / w[2] / 1e3, eng.host_stats()["chunks"]))
        for a in big + [ok_h, st_h]:
            eng.host_free(a)

# the hash alone: 2^20 rows of 112 bytes (two blocks)
nh = 1 << 20
m = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=(nh, 112), dtype=np.uint8)).to(dev)
out = torch.empty((nh, 64), dtype=torch.uint8, device=dev)
t = timed(lambda: eng.sha512_dev(m, 112, None, 112, out, nh))
torch.cuda.synchronize()
want = hashlib.sha512(m[12345].cpu().numpy().tobytes()).digest()
assert out[12345].cpu().numpy().tobytes() == want
clock = clock_under(lambda: eng.sha512_dev(m, 112, None, 112, out, nh))
print("sha512_dev, 2^20 rows of 112 bytes (two blocks each): %s   %.1f M hashes/s   %.1f GB/s of message bytes   clock under load %.0f MHz" % (
    fmt(t), nh / t[0] / 1e3, nh * 112 / t[0] / 1e6, clock["mhz"]))
print("  VALU issue bound for I instructions per block: 256 CUs x 4 SIMDs x clock / 4 / (2 I) hashes/s (I from tools/isa_stats.py, DESIGN.md section 5)")
eng.close()
