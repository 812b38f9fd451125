#!/usr/bin/env python3
"""Writes the measured numbers of DESIGN.md section 6 and of README.md from the committed bench line of the round, so that the documents
and the profile they cite cannot drift apart (and quote the DRIVER'S protocol, not the best run of the round: VERDICT r4 item 2).

    python tools/sync_design_numbers.py            # rewrite the blocks between the BEGIN / END markers
    python tools/sync_design_numbers.py --check    # exit 1 if a block differs from what the profile says; writes nothing

Sources, in this order:
  1. the DRIVER'S own record of the newest round, BENCH_rNN.json at the repo root, when its `parsed` line exists -- stated first, with the
     build id it was taken on (it is the previous round's build until the driver has run this one);
  2. profiles/r06_bench_driver_args_run{1,2,3}.full.json = the full records (bench_full.json) of three runs of
     `python bench.py --full --steps 20 --warmup 5` on one MI355X by the builder; the tables are run 1's.
"""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join("profiles", "r06_bench_driver_args_run1.full.json")
RUNS = [os.path.join("profiles", "r06_bench_driver_args_run%d.full.json" % k) for k in (2, 3)]
BEGIN = "<!-- BEGIN numbers (tools/sync_design_numbers.py) -->"
END = "<!-- END numbers -->"


def e8(v):
    return "%.2f×10⁸" % (v / 1e8)


def ms(v):
    return ("%.3f" % v) if v < 1 else ("%.2f" % v)


def design_block(d):
    lib = d["config"]["library"]
    rows = [("cfg2 (headline): 2¹⁶ variable-base `MUL_endo(m, P)`", d, d["roofline"], d["valu_roofline"], d.get("ct_select", {}).get("cfg2"))]
    names = {"cfg3": "cfg3: 2²⁰ fixed-base `MUL_windowed(m, G, table)`", "cfg4": "cfg4: 2¹⁹ exchanges (comb keygen + `DH_endo`)",
             "cfg5": "cfg5: 2¹⁷ mixed 50/50 `MUL_endo`, work-queue kernel"}
    for k in ("cfg3", "cfg4", "cfg5"):
        r = d["configs"][k]
        rows.append((names[k], r, r["roofline"], r["valu_roofline"], d.get("ct_select", {}).get(k)))
    out = [driver_sentence(lib["build_id"]), "",
           "Build `%s`, `%s` (+ runs 2, 3). The headline of the builder's three runs of the same protocol:" % (lib["build_id"], SOURCE), runs_sentence(d) + ".", "",
           "| configuration (per GPU) | units/s | ms / step | in-kernel clock | cycles / unit | `issue` | algorithmic / executed frac | traffic vs algorithmic | constant-time |",
           "|---|---|---|---|---|---|---|---|---|"]
    for name, r, roof, valu, ct in rows:
        clk = r["clock"]
        issue = valu["issue"]["frac"]
        traffic = roof["traffic"]
        alg = roof["algorithmic_bytes_per_launch"]
        out.append("| %s | **%s** | %s | %.0f MHz | %.2f | %s | %.3f / %.3f | %s | %s |" % (
            name, e8(r["value"]), ms(r["ms_per_step"]), clk["in_kernel_mhz"], r["cycles_per_unit"],
            "%.2f" % issue if issue is not None else "—", valu["algorithmic_frac"], valu["executed_frac"],
            "%.0f MB vs %.0f MB (%.1f×)" % (traffic / 1e6, alg / 1e6, traffic / alg) if traffic else "—",
            "×%.2f" % ct["ratio_vs_default"] if ct else "—"))
    p = d["pcie_inclusive"]
    big = p["at_2^20"]
    out += ["", "Host-array calls (`pcie_inclusive`: first H2D byte to last D2H byte of the synchronous call, pinned arrays, median at the sustained clock):", "",
            "| call | 2¹⁶ elements | 2²⁰ elements |", "|---|---|---|",
            "| R1 in / out, 352 B | %s ms = %s/s | %s ms = **%s/s** (%d chunks) |" % (ms(p["ms_per_step"]), e8(p["value"]), ms(big["r1"]["ms_per_step"]), e8(big["r1"]["value"]), big["r1"]["chunks"]),
            "| affine in / out, 160 B | %s ms = %s/s | %s ms = **%s/s** (%d chunks) |" % (ms(p["affine"]["ms_per_step"]), e8(p["affine"]["value"]), ms(big["affine"]["ms_per_step"]), e8(big["affine"]["value"]), big["affine"]["chunks"]),
            "| 32-byte points in / out, 97 B | %s ms = %s/s | %s ms = **%s/s** (%d chunks) |" % (ms(p["bytes"]["ms_per_step"]), e8(p["bytes"]["value"]), ms(big["bytes"]["ms_per_step"]), e8(big["bytes"]["value"]), big["bytes"]["chunks"]),
            ""]
    if "ct_r1" in big:
        c = big["ct_r1"]
        out += ["The 2²⁰ raw-R1 call on the constant-time context: %s ms = %s/s in %d chunks planned with its own measured %.2f ns per element — %.3f of its floor (constant-time kernels"
                % (ms(c["ms_per_step"]), e8(c["value"]), c["chunks"], c["planned_kernel_ns_per_elem"], c["over_floor"]),
                "device-resident for 2²⁰ + one generation's copy in and out = %s ms)." % ms(c["floor_ms"]), ""]
    hosts = []
    for k, what in (("cfg3", "cfg3's call (scalars in, R1 out)"), ("cfg4", "cfg4's exchange call"), ("cfg5", "cfg5's mixed call")):
        q = d["configs"][k]["pcie_inclusive"]
        extra = ""
        if "keygen_through_the_comb" in q:
            extra = ", %s ms with the keygen half through the comb" % ms(q["keygen_through_the_comb"]["ms_per_step"])
        hosts.append("%s %s ms (pageable caller %s)%s" % (what, ms(q["ms_per_step"]), ms(q["pageable_caller"]["ms_per_step"]), extra))
    out.append("Other configurations through their host-array calls:")
    out.append("")
    out += ["* " + h for h in hosts]
    out.append("")
    sw = d.get("size_sweep")
    if sw:
        sizes = ("1", "1024", "16384", "32768", "65536", "65792", "98304")
        out.append("`size_sweep`, ms per device-resident `MUL_endo` call at %s elements:" % " / ".join(format(int(s), ",").replace(",", " ") for s in sizes))
        out.append("%s; t(65 792) / t(65 536) = %.2f." % (" / ".join("%.3f" % sw[s] for s in sizes), sw["t(65792)/t(65536)"]))
    c = d.get("cpu_baseline")
    if c:
        out.append("CPU baseline (`kind: port`): pure-Python oracle %.3g mults/s on %d of the box's %d cores (%d granted, cap %d) = %.0f per core — the reference's own code does"
                   % (c["value"], c["cores"], c["host_cores_total"], c["host_cores_granted"], c["cores_cap"], c["per_core"]))
        out.append("%.0f per core (SURVEY §6): the port is faster than what it restates; C restatement %.3g/s on %d threads." % (
            c["per_core_reference_survey"], c["c_restatement"]["value"], c["c_restatement"]["threads"]))
    return "\n".join(out)


def earlier_runs():
    """The other runs of the protocol on this round's build (RUNS)."""
    runs = []
    for rel in RUNS:
        path = os.path.join(ROOT, rel)
        if os.path.exists(path):
            with open(path) as fh:
                runs.append(json.load(fh))
    return runs


def runs_sentence(d):
    runs = [d] + earlier_runs()
    return "; ".join("%s at %.0f MHz = %.2f cycles per element" % (e8(r["value"]), r["clock"]["in_kernel_mhz"], r["cycles_per_unit"]) for r in runs)


PINNED_ROUND = None          # --check: the driver's record the committed documents NAME (BENCH_rNN), not whichever is newest on disk


def driver_record():
    """(round number, parsed line) of the newest BENCH_rNN.json at the repo root that the driver could parse, or None.  Under --check the
    record is the one the documents were generated from: the driver drops BENCH_rNN.json of THIS round into the tree after the last commit,
    and the committed documents cannot quote a file that did not exist yet (a note on stderr says so; the check still passes)."""
    best = None
    for path in glob.glob(os.path.join(ROOT, "BENCH_r*.json")):
        m = re.search(r"BENCH_r(\d+)\.json$", path)
        try:
            with open(path) as fh:
                rec = json.load(fh)
        except (OSError, ValueError):
            continue
        if not (m and isinstance(rec.get("parsed"), dict) and "value" in rec["parsed"]):
            continue
        rnd = int(m.group(1))
        if PINNED_ROUND is not None:
            if rnd == PINNED_ROUND:
                return (rnd, rec["parsed"])
            if rnd > PINNED_ROUND:
                print("note: BENCH_r%02d.json is newer than the record the documents quote (BENCH_r%02d): run tools/sync_design_numbers.py to quote it"
                      % (rnd, PINNED_ROUND), file=sys.stderr)
            continue
        if best is None or rnd > best[0]:
            best = (rnd, rec["parsed"])
    return best


def driver_sentence(build_id):
    rec = driver_record()
    if rec is None:
        return "**Driver's record:** none parsed yet."
    rnd, line = rec
    cfg = line.get("config") or {}
    theirs = cfg.get("build_id") or (cfg.get("library") or {}).get("build_id")
    roof = line.get("roofline") or {}
    same = theirs == build_id
    return ("**Driver's record (`BENCH_r%02d.json.parsed`, %s):**\n%s %s at %s ms per step, `roofline.frac` %s.%s" % (
        rnd, "this build" if same else "round %d's build, the newest record the driver could parse — round 5's 22 KB line was not" % rnd,
        e8(line["value"]), line.get("unit", ""), ms(line["ms_per_step"]), roof.get("frac"),
        "" if same else "\nThe driver has not run this round's build yet; what it will read is the compact line the figures below come from."))


def readme_block(d):
    c = d["configs"]
    big = d["pcie_inclusive"]["at_2^20"]
    vals = [r["value"] for r in [d] + earlier_runs()]
    head = e8(d["value"]) if e8(min(vals)) == e8(max(vals)) else "%.2f–%s" % (min(vals) / 1e8, e8(max(vals)))
    return ("%s\n\n"
            "Numbers of `python bench.py --full --steps 20 --warmup 5` — the driver's step counts — on one MI355X (`%s`). Boxes of the pool hold clocks\n"
            "several percent apart under the same kernel, so the line carries the clock of the timed steps and cycles per unit; the builder's three runs:\n"
            "%s.\n"
            "**%s** variable-base scalar multiplications per second at a batch of 2¹⁶ (device-resident;\n"
            "%s/s from pinned host arrays at 2²⁰, PCIe included), %s fixed-base `MUL_windowed`/s, %s Diffie-Hellman exchanges/s,\n"
            "%s/s on the 50/50 fixed / variable mix (one persistent kernel pulling work items off a device-side queue), every output checked\n"
            "bit-exact against the C restatement of the reference in the same run; the pure-Python path does %.3g/s on %d cores of the same box." % (
                driver_sentence(d["config"]["library"]["build_id"]), SOURCE, runs_sentence(d), head, e8(big["r1"]["value"]), e8(c["cfg3"]["value"]), e8(c["cfg4"]["value"]),
                e8(c["cfg5"]["value"]), d["cpu_baseline"]["value"], d["cpu_baseline"]["cores"]))


def main(argv):
    with open(os.path.join(ROOT, SOURCE)) as fh:
        d = json.load(fh)
    check = "--check" in argv
    bad = []
    if check:                                    # pin the driver's record to the one the committed documents name
        global PINNED_ROUND
        m = re.search(r"BENCH_r(\d+)\.json\.parsed", open(os.path.join(ROOT, "DESIGN.md")).read())
        PINNED_ROUND = int(m.group(1)) if m else None
    for path, block in (("DESIGN.md", design_block(d)), ("README.md", readme_block(d))):
        full = os.path.join(ROOT, path)
        text = open(full).read()
        m = re.search(re.escape(BEGIN) + r"\n(.*?)" + re.escape(END), text, re.S)
        if not m:
            bad.append("%s has no numbers block" % path)
            continue
        new = text[:m.start(1)] + block + "\n" + text[m.end(1):]
        if new != text:
            if check:
                bad.append("%s: the numbers block is not what %s says" % (path, SOURCE))
            else:
                open(full, "w").write(new)
                print("updated", path)
    for b in bad:
        print(b, file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
