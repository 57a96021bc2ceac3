#!/usr/bin/env python3
"""Timing of the generic quotient kernel of caller-defined AIRs (plonky3-mobile_amd/air.py, csrc/air.hip) on an MI355X.

  python tools/air_bench.py            runs the three measurements as child processes and writes profiles/air_quotient_bench.txt
  python tools/air_bench.py work ...   the workload itself (what the children run)
  --keep DIR                           keeps the profiler's files; `python tools/air_bench.py report --keep DIR` writes the report again

  1. the generic kernel on the fib program at 2^20 rows beside fib_quotient_kernel of a FibAirProver.prove, in ONE process under
     `rocprofv3 --kernel-trace` (medians of the dispatches): the price of interpretation;
  2. AIR (C) of the tests (width 70, degree 4, 4 chunks) at 2^16 rows, blowup 2, in the same trace, beside a device-to-device copy of
     the bytes it reads and writes (every LDE word of the quotient domain once, every quotient word once) timed with device events
     in a run without the profiler (a third process: the same call timed there with events is printed beside it, so the two
     processes can be compared): the yardstick of profiles/pcs_hiding_open_bench.txt;
  3. VALU instructions per row from a separate `rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES` run (SQ_INSTS_VALU counts per wave, a wave's
     instruction serves its 64 rows, so instructions per row = SQ_INSTS_VALU / SQ_WAVES) beside the count the program implies."""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
from air_ref import C_WIDTH, air_c  # noqa: E402  (AIR (C) of the tests)

P = 0x78000001
FIB_LOG_N, C_LOG_N = 20, 16
FIB_FRI, C_FRI = (1, 0, 100, 16), (2, 0, 100, 16)


def _monty(rng, n):
    return ((rng.integers(0, P, n, dtype=np.uint64) << 32) % P).astype(np.uint32)


def implied_instructions(air):
    """VALU instructions per row the PROGRAM implies: 5 per product, 2 per addition or subtraction, 4 products per constraint for
    the fold (two constraints share a reduction: 4 x 4 instructions each), and the fixed part: x_i (2 products), one field
    inversion (31 squarings and 29 products), 5 products for the two selectors, 4 for the division by Z_H"""
    ops = air.code[:, 0]
    mul, lin, k = int((ops == 2).sum()), int(((ops == 0) | (ops == 1)).sum()), air.n_constraints
    return 5 * mul + 2 * lin + 16 * k + 5 * (2 + 60 + 5 + 4)


def _timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def work(a):
    """the fib prover's proofs, then the generic kernel on the fib program over the same trace's LDE, then AIR (C); --events: device
    events around each call and the copy yardstick (the run without the profiler)"""
    import torch
    p3 = load_package()
    rng = np.random.default_rng(1)
    alpha = _monty(rng, 4)
    pr = p3.FibAirProver(FIB_LOG_N, params=p3.FriParameters(*FIB_FRI))
    for _ in range(a.warmup + a.reps):
        pr.prove(0, 1)
    pr.close()
    out = []
    # fib program, 2^20 rows, blowup 2
    fib = p3.fibonacci_air()
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*FIB_FRI))
    _, data = pcs.commit([(p3.generate_trace_rows(0, 1, 1 << FIB_LOG_N), None)])
    lde = pcs.get_evaluations_on_domain(data, 0, FIB_LOG_N)
    pis = _monty(rng, 3)
    ms = _timed(lambda: fib.quotient(lde, FIB_LOG_N, FIB_FRI[0], pis, alpha), a.warmup, a.reps)
    out.append("events fib_program_2^20 median_ms %.4f min_ms %.4f n %d" % (statistics.median(ms), min(ms), len(ms)))
    data.free()
    pcs.free()
    # AIR (C), 2^16 rows, blowup 2 -> 4 chunks over 2^18 rows
    c = air_c(p3)
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*C_FRI))
    trace = torch.randint(0, P, (1 << C_LOG_N, C_WIDTH), dtype=torch.int32, device="cuda")
    _, data = pcs.commit([(trace, None)])
    lde = pcs.get_evaluations_on_domain(data, 0, C_LOG_N + c.log_quotient_degree)
    pis = _monty(rng, 1)
    ms = _timed(lambda: c.quotient(lde, C_LOG_N, C_FRI[0], pis, alpha), a.warmup, a.reps)
    out.append("events air_C_2^16 median_ms %.4f min_ms %.4f n %d" % (statistics.median(ms), min(ms), len(ms)))
    if a.events:
        qn = (1 << C_LOG_N) << c.log_quotient_degree
        nbytes = 4 * qn * C_WIDTH + 16 * qn  # read + written, every word once
        src = torch.empty(nbytes // 8, dtype=torch.int32, device="cuda")  # half the bytes read, half written
        dst = torch.empty_like(src)
        ms = _timed(lambda: dst.copy_(src), a.warmup, a.reps)
        out.append("events copy_of_air_C_bytes bytes %d median_ms %.4f min_ms %.4f n %d" % (nbytes, statistics.median(ms), min(ms), len(ms)))
    data.free()
    pcs.free()
    out.append("program fib instructions %d constraints %d slots %d implied_valu_per_row %d" % (fib.n_instructions, fib.n_constraints, fib.n_slots, implied_instructions(fib)))
    out.append("program air_C instructions %d constraints %d slots %d implied_valu_per_row %d" % (c.n_instructions, c.n_constraints, c.n_slots, implied_instructions(c)))
    print("\n".join(out))


def _grid(r):
    return int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)


def _kernel_medians(d):
    """{(kernel, work-items): (median us, dispatches)} of a --kernel-trace directory"""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    acc = {}
    for r in (csv.DictReader(open(files[0])) if files else []):
        name = r["Kernel_Name"]
        key = "air_kernel<0>" if "air_kernel<0>" in name else "fib_quotient_kernel" if "fib_quotient_kernel" in name else None
        if key:
            acc.setdefault((key, _grid(r)), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (statistics.median(v), len(v)) for k, v in acc.items()}


def _valu_per_row(d):
    """{work-items: SQ_INSTS_VALU / SQ_WAVES of the air_kernel<0> dispatches} of a --pmc directory"""
    files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    acc = {}
    for r in (csv.DictReader(open(files[0])) if files else []):
        if "air_kernel<0>" in r["Kernel_Name"]:
            c = acc.setdefault(_grid(r), {})
            c[r["Counter_Name"]] = c.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    return {g: c["SQ_INSTS_VALU"] / c["SQ_WAVES"] for g, c in acc.items() if c.get("SQ_WAVES")}


def report(trace_dir, pmc_dir, events_text, warmup, reps):
    ev = {ln.split()[1]: ln.split() for ln in events_text.splitlines() if ln.startswith("events ")}
    prog = {ln.split()[1]: ln.split() for ln in events_text.splitlines() if ln.startswith("program ")}
    val = lambda words, key: float(words[words.index(key) + 1])
    km, vr = _kernel_medians(trace_dir), _valu_per_row(pmc_dir)
    out = ["# tools/air_bench.py: the generic quotient kernel (csrc/air.hip air_kernel<0>) on an MI355X; kernel times are medians of the",
           "# dispatches of one process under rocprofv3 --kernel-trace (%d warm-up + %d timed calls each); the copy is timed with device" % (warmup, reps),
           "# events in a run without the profiler; instruction counts come from a separate rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES run"]
    n_fib, qn_c = 1 << FIB_LOG_N, (1 << C_LOG_N) << 2
    a, f = km.get(("air_kernel<0>", n_fib)), km.get(("fib_quotient_kernel", n_fib))
    out.append("1. fib program, 2^%d rows: air_kernel<0> %s; fib_quotient_kernel %s" % (
        FIB_LOG_N, "median %.1f us of %d dispatches" % a if a else "not in the trace", "median %.1f us of %d dispatches" % f if f else "not in the trace"))
    if a and f:
        out.append("   ratio generic / specialised: %.2f" % (a[0] / f[0]))
    c = km.get(("air_kernel<0>", qn_c))
    out.append("2. AIR (C), 2^%d rows x %d columns, blowup 2 (2^%d quotient rows, 4 chunks): air_kernel<0> %s" % (
        C_LOG_N, C_WIDTH, C_LOG_N + 2, "median %.1f us of %d dispatches" % c if c else "not in the trace"))
    if "copy_of_air_C_bytes" in ev:
        w = ev["copy_of_air_C_bytes"]
        nbytes, ms = val(w, "bytes"), val(w, "median_ms")
        out.append("   bytes read + written (every word once): %d; a device-to-device copy of as many bytes (half read, half written): median %.1f us"
                   " -> %.0f GB/s" % (nbytes, ms * 1e3, nbytes / ms / 1e6))
        if c:
            out.append("   the kernel moves them at %.0f GB/s: %.2f x the copy's time" % (nbytes / (c[0] * 1e3), c[0] / (ms * 1e3)))
        out.append("   (the copy's two buffers of %.0f MB are rewritten in every repetition and fit the 256 MB last-level cache: its rate is cache-assisted,"
                   " not an HBM figure; it is the lower bound a kernel moving these bytes could approach here)" % (nbytes / 2e6))
    for name, g, label in (("fib", n_fib, "fib program"), ("air_C", qn_c, "AIR (C)")):
        implied = val(prog[name], "implied_valu_per_row") if name in prog else float("nan")
        got = vr.get(g)
        out.append("3. %s: VALU instructions per row %s; the program implies %.0f (%d instructions, %d constraints)" % (
            label, "%.0f (SQ_INSTS_VALU / SQ_WAVES)" % got if got else "not measured", implied,
            val(prog[name], "instructions") if name in prog else 0, val(prog[name], "constraints") if name in prog else 0))
    for name in ("fib_program_2^20", "air_C_2^16"):
        if name in ev:
            out.append("   call time with device events, upload included (%s): median %.1f us" % (name, val(ev[name], "median_ms") * 1e3))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="all", choices=["all", "work", "report"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--events", action="store_true")
    ap.add_argument("--keep", metavar="DIR", help="keep the profiler's output there (trace/, pmc/, events.txt); `report` reads it again")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "air_quotient_bench.txt"))
    a = ap.parse_args()
    if a.mode == "work":
        return work(a)
    tmp = a.keep or tempfile.mkdtemp()
    t, p, e = os.path.join(tmp, "trace"), os.path.join(tmp, "pmc"), os.path.join(tmp, "events.txt")
    if a.mode == "all":
        if not shutil.which("rocprofv3"):
            sys.exit("air_bench: rocprofv3 is not on the PATH")
        os.makedirs(tmp, exist_ok=True)
        me = [sys.executable, os.path.abspath(__file__), "work"]
        full = ["--warmup", str(a.warmup), "--reps", str(a.reps)]
        # three fresh processes, one after the other; a failure ends the run
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", t, "--"] + me + full, check=True, timeout=400,
                       stdout=subprocess.DEVNULL)
        subprocess.run(["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_WAVES", "--output-format", "csv", "-d", p, "--"] + me + ["--warmup", "1", "--reps", "2"],
                       check=True, timeout=400, stdout=subprocess.DEVNULL)
        with open(e, "w") as f:
            f.write(subprocess.run(me + full + ["--events"], check=True, timeout=400, stdout=subprocess.PIPE, text=True).stdout)
    text = report(t, p, open(e).read(), a.warmup, a.reps)
    if not a.keep:
        shutil.rmtree(tmp, ignore_errors=True)
    sys.stdout.write(text)
    with open(a.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
