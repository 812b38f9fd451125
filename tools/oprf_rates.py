#!/usr/bin/env python3
"""Device-resident rates of the oblivious-PRF calls beside the compositions of older calls they replace.

    python tools/oprf_rates.py [--out profiles/oprf_rates.txt] [--sizes 65536,1048576] [--rounds 3]

Per size: every call and, in the same run and alternating with it, its composition
    blind     hash_to_curve_dev (32 bytes) + mul_bytes_dev
    evaluate  dh_bytes_dev with the key on n scalar rows
    finalize  mul_bytes_dev (inverses supplied) + sha512_dev over ready-made strings -- the excess is the price of the inversion
and scalar_inv_dev at every shipped K (Engine.set_scinv_group on an engine of its own).  One measurement is 5 warm-up and 20 timed steps between two
HIP events, bracketed by diag_clock_begin / _stop / _end as bench.py does; every row is measured `rounds` times, the rounds of all rows
interleaved, and reported as the median with the spread (max - min) over its rounds -- the run-to-run noise the comparisons are read
against.  Before anything is timed the outputs are compared with the compositions' at the size timed.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FOURQ_DEBUG_ROUTES", "1")          # for Engine.set_scinv_group on the per-K engines only

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fourq_amd import Engine, codec  # noqa: E402
from fourq_amd.constants import N  # noqa: E402

WARMUP, STEPS = 5, 20
DST = b"FourQ-OPRF-V01-rates"
STRIDE = 32                                               # a password-sized message: F's string is one block
SHIPPED_K = (1, 8, 16)


def dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to("cuda:0")


def measure(eng, step):
    for _ in range(WARMUP):
        step()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.sync()
    stream = torch.cuda.current_stream()
    eng.diag_clock_begin()
    eng.sync()
    ev0.record(stream)
    for _ in range(STEPS):
        step()
    eng.sync()
    ev1.record(stream)
    eng.diag_clock_stop()
    torch.cuda.synchronize()
    try:
        mhz = eng.diag_clock_end()["mhz"]
    except Exception:
        mhz = float("nan")
    return ev0.elapsed_time(ev1) / STEPS, mhz


def rows_for(eng, n, rounds, lines):
    rng = np.random.default_rng(n)
    m = rng.integers(0, 256, size=(n, STRIDE), dtype=np.uint8)
    lens = rng.integers(8, STRIDE + 1, size=n, dtype=np.uint32)
    r = rng.integers(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    key = codec.pack_scalars([0x1234567890ABCDEF << 128 | 0xFEDCBA])[0]
    d_m, d_len, d_r, d_keys = dev(m), dev(lens), dev(r), dev(np.tile(key, (n, 1)))
    u8 = lambda cols: torch.empty((n, cols), dtype=torch.uint8, device="cuda:0")
    pts32, blinded, blinded2, evaluated, evaluated2, e32, out, out2, direct = u8(32), u8(32), u8(32), u8(32), u8(32), u8(32), u8(64), u8(64), u8(64)
    st, st2 = torch.empty(n, dtype=torch.uint8, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_inv = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
    eng.reserve(n)
    tail = b"Finalize" + DST + bytes([len(DST)])
    width = 32 + STRIDE + len(tail)
    d_flen = dev((32 + lens + len(tail)).astype(np.uint32))

    new_blind = lambda: eng.oprf_blind_dev(d_m, STRIDE, d_len, 0, d_r, blinded, st, n, dst=DST)
    def old_blind():
        eng.hash_to_curve_dev(d_m, STRIDE, d_len, 0, pts32, n, dst=DST)
        eng.mul_bytes_dev(d_r, pts32, blinded2, st2, n)
    new_evaluate = lambda: eng.oprf_evaluate_dev(key, blinded, evaluated, st, n)
    old_evaluate = lambda: eng.dh_bytes_dev(d_keys, blinded, None, evaluated2, st2, n)
    new_finalize = lambda: eng.oprf_finalize_dev(d_m, STRIDE, d_len, 0, d_r, evaluated, out, st, n, dst=DST)
    new_eval = lambda: eng.oprf_eval_dev(key, d_m, STRIDE, d_len, 0, direct, st, n, dst=DST)

    # correctness at this size, against the composition: blind, evaluate, then the strings of F built on the host from the composition's E
    new_blind(); old_blind(); eng.sync()
    assert torch.equal(blinded, blinded2) and not st.any()
    new_evaluate(); old_evaluate(); eng.sync()
    assert torch.equal(evaluated, evaluated2) and not st.any()
    eng.scalar_inv_dev(d_r, d_inv, n); eng.sync()
    inv = d_inv.cpu().numpy().view(np.uint64)
    probe = rng.integers(0, n, size=64)
    assert all(int(a) == pow(int(b) % N, -1, N) for a, b in zip(codec.unpack_scalars(inv[probe]), codec.unpack_scalars(r[probe])))
    eng.mul_bytes_dev(d_inv, evaluated, e32, st2, n); eng.sync()
    strings = np.zeros((n, width), dtype=np.uint8)
    strings[:, :32] = e32.cpu().numpy()
    for ln in range(STRIDE + 1):
        sel = np.flatnonzero(lens == ln)
        strings[sel[:, None], 32 + np.arange(ln)[None, :]] = m[sel, :ln]
        strings[sel[:, None], 32 + ln + np.arange(len(tail))[None, :]] = np.frombuffer(tail, dtype=np.uint8)
    d_strings = dev(strings)
    def old_finalize():
        eng.mul_bytes_dev(d_inv, evaluated, e32, st2, n)
        eng.sha512_dev(d_strings, width, d_flen, 0, out2, n)
    new_finalize(); old_finalize(); new_eval(); eng.sync()
    assert torch.equal(out, out2) and torch.equal(out, direct) and not st.any()

    table = [("blind", eng, new_blind), ("  hash_to_curve + mul_bytes", eng, old_blind), ("evaluate", eng, new_evaluate), ("  dh_bytes", eng, old_evaluate),
             ("finalize", eng, new_finalize), ("  mul_bytes + sha512", eng, old_finalize), ("eval", eng, new_eval),
             ("mul_bytes alone (the ladder beside the inversion)", eng, lambda: eng.mul_bytes_dev(d_inv, evaluated, e32, st2, n))]
    engines = []
    for k in SHIPPED_K:
        e = Engine(0)
        e.set_scinv_group(k)
        engines.append(e)
        table.append(("scalar_inv K=%d" % k, e, (lambda e: lambda: e.scalar_inv_dev(d_r, d_inv, n))(e)))
    table.append(("scalar_inv (K by batch size)", eng, lambda: eng.scalar_inv_dev(d_r, d_inv, n)))
    ms = {name: [] for name, _, _ in table}
    mhz = {name: [] for name, _, _ in table}
    for _ in range(rounds):
        for name, e, step in table:
            t, c = measure(e, step)
            ms[name].append(t)
            mhz[name].append(c)
    lines.append("n = %d  (%d rounds of %d + %d steps, rows interleaved; ms per step: median, spread = max - min over the rounds)" % (n, rounds, WARMUP, STEPS))
    for name, _, _ in table:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        lines.append("  %-52s %9.4f ms  spread %7.4f  %8.2f ns/row  %6.0f MHz" % (name, med, v[-1] - v[0], med * 1e6 / n, float(np.nanmedian(mhz[name]))))
    for e in engines:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oprf_rates.txt"))
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    eng = Engine(0)
    lines = ["oblivious PRF, device-resident, build %s, messages of 8..%d bytes in a %d-byte stride, DST of %d bytes" % (eng.build_id, STRIDE, STRIDE, len(DST))]
    for n in (int(s) for s in args.sizes.split(",")):
        rows_for(eng, n, args.rounds, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
