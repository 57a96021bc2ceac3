#!/usr/bin/env python3
"""Timing of the device TwoAdicFriPcs (plonky3-mobile_amd/pcs.py): commit and open of four shape sets at 2 opening points, with
device timestamps (events on the stream the PCS enqueues on), warm-up, repetitions and the spread.

  python tools/pcs_bench.py                       every shape set: commit / open times, the copy yardstick, the fib comparison
  python tools/pcs_bench.py --shape NAME --plain   one shape set, opens only, no yardstick: the run to put under
                                                   `rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python ...`
  python tools/pcs_bench.py --merge DIR ...        adds the per-kernel split of such runs (DIR/NAME/**/*kernel_trace.csv)
  -o FILE                                          where the report goes (default profiles/pcs_open_bench.txt)

Algorithmic bytes of the streaming kernels: reduced openings 4*big*w (every LDE word once), opened values 4*h*w (the low coset
once), inverse denominators and ro 16*big*(K + 1).  The yardstick is a device-to-device copy of the same byte count timed in the
same run (bytes counted once, as for the kernels), not a specification figure."""
import argparse
import glob
import csv
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

P = 0x78000001
SHAPES = {  # name -> (log_h, rounds: [[(width, points)]]), points index the two points z0, z1
    "fib_2^20x2+4": (20, [[(2, (0, 1))], [(4, (0,))]]),
    "2^20x32": (20, [[(32, (0, 1))]]),
    "2^20x64": (20, [[(64, (0, 1))]]),
    "2^16x2633": (16, [[(2633, (0, 1))]]),
}
FRI = (1, 0, 100, 16)  # blowup 2, the benchmark's FRI parameters


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


def _fmt(ms):
    return "median %.3f ms  min %.3f  max %.3f  (n=%d)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def _copy_rate(nbytes, warmup, reps):
    import torch
    src = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    ms = _timed(lambda: dst.copy_(src), warmup, reps)
    return nbytes / statistics.median(ms) / 1e6  # GB/s


def run_shape(p3, name, warmup, reps, plain, out):
    import torch
    log_h, rounds = SHAPES[name]
    h, big = 1 << log_h, 1 << (log_h + FRI[0])
    rng = np.random.default_rng(1)
    z = [((rng.integers(0, P, 4, dtype=np.uint64) << 32) % P).astype(np.uint32) for _ in range(2)]
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*FRI), "poseidon2")
    mats = [[torch.randint(0, P, (h, w), dtype=torch.int32, device="cuda") for w, _ in r] for r in rounds]
    commit = lambda: [pcs.commit([(m, None) for m in r]) for r in mats]
    if not plain:
        def commit_and_free():
            for _, d in commit():
                d.free()
        out.append("%-14s commit (LDE + tree, all rounds): %s" % (name, _fmt(_timed(commit_and_free, warmup, reps))))
    datas = [d for _, d in commit()]
    arg = [(d, [[z[i] for i in pts] for _, pts in r]) for d, r in zip(datas, rounds)]
    ms = _timed(lambda: pcs.open(arg, p3.Challenger()), warmup, reps)
    out.append("%-14s open: %s" % (name, _fmt(ms)))
    if not plain:
        wsum = sum(w for r in rounds for w, _ in r)
        for what, nbytes in (("reduced openings 4*big*w", 4 * big * wsum), ("opened values 4*h*w", 4 * h * wsum),
                             ("denominators + ro 16*big*(K+1)", 16 * big * 3)):
            out.append("%-14s   %-32s %12d bytes; a device-to-device copy of them runs at %.0f GB/s" % (name, what, nbytes, _copy_rate(nbytes, warmup, reps)))
    for d in datas:
        d.free()
    pcs.free()


def fib_comparison(p3, warmup, reps, out):
    """the PCS calls of a fib proof (commit trace, commit quotient, open; the quotient's values are given: its arithmetic is the AIR's,
    not the PCS's) beside FibAirProver.prove, 2^20 rows"""
    import torch
    log_n = 20
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*FRI), "poseidon2")
    trace = p3.generate_trace_rows(0, 1, 1 << log_n)
    quot = torch.randint(0, P, (1 << log_n, 4), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(2)
    z = [((rng.integers(0, P, 4, dtype=np.uint64) << 32) % P).astype(np.uint32) for _ in range(2)]

    def through():
        _, dt = pcs.commit([(trace, None)])
        _, dq = pcs.commit([(quot, p3.GENERATOR_MONTY)])
        pcs.open([(dt, [[z[0], z[1]]]), (dq, [[z[0]]])], p3.Challenger())
        dt.free()
        dq.free()
    a = _timed(through, warmup, reps)
    pr = p3.FibAirProver(log_n, params=p3.FriParameters(*FRI))
    b = _timed(lambda: pr.prove(0, 1), warmup, reps)
    pr.close()
    out.append("fib 2^20 through the PCS (2 commits + open, quotient values given): %s" % _fmt(a))
    out.append("fib 2^20 FibAirProver.prove:                                        %s" % _fmt(b))
    out.append("ratio of the medians (general path / fib prover): %.2f" % (statistics.median(a) / statistics.median(b)))


def merge(prof_dir, out):
    """per-kernel split of the opens of a profiled --plain run: the dispatches from the first pcs_inv_denoms_kernel on (what comes
    before is the upload and the one commit), summed per kernel and divided by the number of opens"""
    for name in SHAPES:
        files = glob.glob(os.path.join(prof_dir, name, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            out.append("%-14s no kernel trace under %s" % (name, prof_dir))
            continue
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
        short = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("p3::", "").split("<")[0]
        first = next(i for i, r in enumerate(rows) if short(r) == "pcs_inv_denoms_kernel")
        rows = rows[first:]
        opens = sum(1 for r in rows if short(r) == "pcs_ts_open_kernel")
        log_h, rounds = SHAPES[name]
        h, big = 1 << log_h, 1 << (log_h + FRI[0])
        wsum = sum(w for r in rounds for w, _ in r)
        algo = {"pcs_reduced": 4 * big * wsum, "pcs_bary": 4 * h * wsum, "pcs_inv_denoms": 16 * big * 2}
        out.append("%-14s kernels of an open, by time (mean of %d opens under rocprofv3 --kernel-trace):" % (name, opens))
        agg = {}
        for r in rows:
            agg[short(r)] = agg.get(short(r), 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        tot = 0.0
        for k, ns in sorted(agg.items(), key=lambda kv: -kv[1]):
            us = ns / opens / 1e3
            tot += us
            line = "%-14s   %-34s %10.1f us" % (name, k, us)
            for key, nbytes in algo.items():
                if k.startswith(key):
                    line += "   %d algorithmic bytes -> %.0f GB/s" % (nbytes, nbytes / (us * 1e3))
            out.append(line)
        out.append("%-14s   %-34s %10.1f us" % (name, "all kernels", tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--merge")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "pcs_open_bench.txt"))
    a = ap.parse_args()
    p3 = load_package()
    out = ["# tools/pcs_bench.py: FRI parameters %s, Poseidon2 hashes, latency profile, 2 opening points; device timestamps,"
           % (FRI,), "# %d warm-up and %d timed repetitions per figure" % (a.warmup, a.reps)]
    for name in ([a.shape] if a.shape else list(SHAPES)):
        run_shape(p3, name, a.warmup, a.reps, a.plain, out)
    if not a.plain:
        fib_comparison(p3, a.warmup, a.reps, out)
    if a.merge:
        merge(a.merge, out)
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if not a.plain:
        with open(a.output, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
