#!/usr/bin/env python3
"""Device-resident times of the batched DLEQ proofs beside the summed times of the existing calls they are composed of.

    python tools/dleq_timing.py [--out profiles/dleq_timing.txt] [--rows 65536] [--group-sizes 1,64] [--rounds 3]

Per group size, in one run and with the rounds of all rows interleaved:
    prove     dleq_prove_dev          beside  msm_bytes_dev (rows) + oprf_evaluate_dev + mul_bytes_dev + comb_mul_dev (groups each)
    verify    dleq_verify_dev         beside  2 x msm_bytes_dev (rows) + double_mul_bytes_dev (groups) + msm_bytes_dev (groups of two)
The difference is what the proofs' own kernels cost: the composite scalars (one hash per row), the challenge (one per group), the split and
the check.  One measurement is 5 warm-up and 20 timed steps between two HIP events; every row is measured `rounds` times and reported as
the median with the spread (max - min) over its rounds.  Before anything is timed, verify must accept what prove made.  A record, not a gate.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fourq_amd import Engine, codec  # noqa: E402
from fourq_amd.constants import Gx, Gy  # noqa: E402

WARMUP, STEPS = 5, 20
DST = b"FourQ-DLEQ-V01-timing"


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
    ev0.record(stream)
    for _ in range(STEPS):
        step()
    eng.sync()
    ev1.record(stream)
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / STEPS


def rows_for(eng, n, group_size, rounds, lines):
    groups = n // group_size
    rng = np.random.default_rng(n + group_size)
    key = codec.pack_scalars([0x1234567890ABCDEF << 128 | 0xFEDCBA])[0]
    pk = eng.dleq_public_key(key)
    msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    rand = lambda rows: dev(rng.integers(0, 2**63, size=(rows, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1))
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda:0")
    blinded, evaluated, st_rows = u8(n, 32), u8(n, 32), u8(n)
    eng.reserve(max(n, 2 * groups))
    eng.dleq_reserve(groups, group_size)
    eng.hash_to_curve_dev(dev(msgs), 32, None, 32, blinded, n, dst=DST)
    eng.oprf_evaluate_dev(key, blinded, evaluated, st_rows, n)
    nonces, d_rows, s_groups, c_groups, pair_sc = rand(groups), rand(n), rand(groups), rand(groups), rand(2 * groups)
    proof, ok, st = u8(groups, 64), u8(groups), u8(groups)
    m32, z32, t32, pair_pt, pk_rows = u8(groups, 32), u8(groups, 32), u8(groups, 32), u8(2 * groups, 32), dev(np.tile(pk, (groups, 1)))
    affine = torch.empty((groups + 1, 8), dtype=torch.int64, device="cuda:0")
    comb_k, st1 = rand(groups + 1), u8(groups + 1)

    prove = lambda: eng.dleq_prove_dev(key, blinded, evaluated, nonces, proof, st, groups, group_size, dst=DST)
    verify = lambda: eng.dleq_verify_dev(pk, blinded, evaluated, proof, ok, st, groups, group_size, dst=DST)
    prove(); verify(); eng.sync()
    assert bool(ok.all()) and not bool(st.any()), "verify must accept what prove made"
    eng.msm_bytes_dev(d_rows, blinded, m32, st, groups, group_size)
    eng.msm_bytes_dev(d_rows, evaluated, z32, st, groups, group_size)
    eng.sync()
    pair_pt.view(groups, 2, 32)[:, 0], pair_pt.view(groups, 2, 32)[:, 1] = m32, z32

    def prove_parts():
        eng.comb_mul_dev(comb_k, None, affine, st1, groups + 1)
        eng.msm_bytes_dev(d_rows, blinded, m32, st, groups, group_size)
        eng.oprf_evaluate_dev(key, m32, t32, st, groups)
        eng.mul_bytes_dev(s_groups, m32, t32, st, groups)

    def verify_parts():
        eng.msm_bytes_dev(d_rows, blinded, m32, st, groups, group_size)
        eng.msm_bytes_dev(d_rows, evaluated, z32, st, groups, group_size)
        eng.double_mul_bytes_dev(s_groups, c_groups, pk_rows, t32, st, groups)
        eng.msm_bytes_dev(pair_sc, pair_pt, t32, st, groups, 2)

    table = [("prove", prove), ("  comb_mul + msm_bytes + oprf_evaluate + mul_bytes", prove_parts), ("verify", verify),
             ("  2 msm_bytes + double_mul_bytes + msm_bytes of two", verify_parts)]
    ms = {name: [] for name, _ in table}
    for _ in range(rounds):
        for name, step in table:
            ms[name].append(measure(eng, step))
    lines.append("rows = %d, group_size = %d, groups = %d  (%d rounds of %d + %d steps, interleaved; ms per step: median, spread = max - min)" % (
        n, group_size, groups, rounds, WARMUP, STEPS))
    for name, _ in table:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        lines.append("  %-54s %9.4f ms  spread %7.4f  %8.2f ns/row" % (name, med, v[-1] - v[0], med * 1e6 / n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dleq_timing.txt"))
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--group-sizes", default="1,64")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    eng = Engine(0)
    g_r1 = codec.pack_point((Gx, Gy, (1, 0), Gx, Gy))             # AffineToR1(Gx, Gy)
    eng.comb_stage(eng.comb_table(g_r1))
    lines = ["batched DLEQ proofs, device-resident, build %s, DST of %d bytes, selection by address" % (eng.build_id, len(DST))]
    for gs in (int(s) for s in args.group_sizes.split(",")):
        rows_for(eng, args.rows, gs, args.rounds, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
