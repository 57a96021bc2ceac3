#!/usr/bin/env python3
"""Timing of the device TwoAdicFriPcs (plonky3-mobile_amd/pcs.py): commit and open of four shape sets at 2 opening points, with
device timestamps (events on the stream the PCS enqueues on), warm-up, repetitions and the spread.

  python tools/pcs_bench.py                       every shape set: commit / open times, the copy yardstick, the fib comparison
  python tools/pcs_bench.py --shape NAME --plain   one shape set, opens only, no yardstick: the run to put under
                                                   `rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python ...`
  python tools/pcs_bench.py --merge DIR ...        adds the per-kernel split of such runs (DIR/NAME/**/*kernel_trace.csv)
  -o FILE                                          where the report goes (default profiles/pcs_open_bench.txt)
  python tools/pcs_bench.py --hiding               the device HidingFriPcs: commit / commit_quotient times, the copy yardstick of the two
                                                   streaming kernels, the hiding fib comparison (default profiles/pcs_hiding_open_bench.txt)
  python tools/pcs_bench.py --hiding --plain       the hiding commits only: the run to put under rocprofv3 --kernel-trace
  python tools/pcs_bench.py --mixed                an open over MIXED heights (2^20 x 16 + 2^18 x 64 + 2^16 x 4, TwoAdicFriPcs(mixed_heights=
                                                   True)) and a same-height 2^20 x 16 open in the same process; the copy yardsticks of the
                                                   fold kernels (default profiles/pcs_mixed_open_bench.txt)
  python tools/pcs_bench.py --mixed --plain        the opens only: the run to put under rocprofv3 --kernel-trace
  python tools/pcs_bench.py --mixed --merge DIR    adds fri_fold_rollin_kernel beside fri_fold_kernel at the same length from DIR/**/*kernel_trace.csv
  python tools/pcs_bench.py --hiding --merge DIR   adds the device times of pcs_randomize_kernel / pcs_blind_kernel from DIR/**/*kernel_trace.csv

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


# ---- mixed heights ----
MIXED = [(20, 16), (18, 64), (16, 4)]  # (log_h, width), one commitment, both points on every matrix
FOLD_BYTES, ROLLIN_BYTES = 48, 64      # per output element: two inputs read and one output written, 16 bytes each; + ro read


def run_mixed(p3, warmup, reps, plain, out):
    import torch
    rng = np.random.default_rng(1)
    z = [((rng.integers(0, P, 4, dtype=np.uint64) << 32) % P).astype(np.uint32) for _ in range(2)]
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*FRI), "poseidon2", mixed_heights=True)
    for name, shape in (("mixed 2^20x16+2^18x64+2^16x4", MIXED), ("same  2^20x16", MIXED[:1])):
        mats = [torch.randint(0, P, (1 << lh, w), dtype=torch.int32, device="cuda") for lh, w in shape]
        if not plain:
            out.append("%-30s commit (LDEs + one tree): %s" % (name, _fmt(_timed(lambda: pcs.commit([(m, None) for m in mats])[1].free(), warmup, reps))))
        _, d = pcs.commit([(m, None) for m in mats])
        arg = [(d, [[z[0], z[1]]] * len(mats))]
        out.append("%-30s open: %s" % (name, _fmt(_timed(lambda: pcs.open(arg, p3.Challenger()), warmup, reps))))
        d.free()
    if not plain:
        for lh, _ in MIXED[1:]:  # the folds that take a roll-in leave 2^(log_h + log_blowup) elements
            half = 1 << (lh + FRI[0])
            for what, per in (("fri_fold_kernel", FOLD_BYTES), ("fri_fold_rollin_kernel", ROLLIN_BYTES)):
                out.append("fold to 2^%d elements: %-22s %10d bytes; a device-to-device copy of them runs at %.0f GB/s"
                           % (lh + FRI[0], what, per * half, _copy_rate(per * half, warmup, reps)))
    pcs.free()


def merge_mixed(prof_dir, out):
    """median device time of the two fold kernels at the lengths that take a roll-in, from a profiled --mixed --plain run (the plain
    kernel's dispatches of that length come from the same-height opens of the same process)"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        out.append("no kernel trace under %s" % prof_dir)
        return
    rows = list(csv.DictReader(open(files[0])))
    grid = lambda r: int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)  # work-items of the launch: one per output element
    for lh, _ in MIXED[1:]:
        half = 1 << (lh + FRI[0])
        for kernel, per in (("fri_fold_kernel", FOLD_BYTES), ("fri_fold_rollin_kernel", ROLLIN_BYTES)):
            ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel + "(" in r["Kernel_Name"].replace("p3::", "") and grid(r) == half]
            if not ns:
                out.append("fold to 2^%d elements: %-22s no dispatch of that length in the trace" % (lh + FRI[0], kernel))
                continue
            us = statistics.median(ns) / 1e3
            out.append("fold to 2^%d elements: %-22s median %8.1f us of %d dispatches under rocprofv3 --kernel-trace; %d bytes -> %.0f GB/s"
                       % (lh + FRI[0], kernel, us, len(ns), per * half, per * half / (us * 1e3)))


# ---- HidingFriPcs ----
HIDING_SHAPES = [(20, 2), (20, 64), (16, 2633)]  # (log_h, w) of a committed matrix
NRC, CHUNKS, MAX_WQ = 4, 4, 2048


def _blind_width(w):
    return min(w, MAX_WQ)  # commit_quotient takes chunks of at most 2048 columns: the widest shape is timed at that width


def hiding_bytes(log_h, w):
    """algorithmic bytes (read + written, each word once) of the two streaming kernels"""
    h, wq = 1 << log_h, _blind_width(w)
    randomize = 4 * (h * w + h * (w + 2 * NRC)) + 4 * 2 * h * (w + NRC)
    blind = 4 * (CHUNKS * h * wq + (CHUNKS - 1) * h * wq) + 4 * CHUNKS * 2 * h * wq
    return randomize, blind


def run_hiding(p3, warmup, reps, plain, out):
    import torch
    for log_h, w in HIDING_SHAPES:
        h, name = 1 << log_h, "2^%dx%d" % (log_h, w)
        pcs = p3.HidingFriPcs(p3.FriParameters(*FRI), "poseidon2")
        m = torch.randint(0, P, (h, w), dtype=torch.int32, device="cuda")
        chunks = [torch.randint(0, P, (h, _blind_width(w)), dtype=torch.int32, device="cuda") for _ in range(CHUNKS)]
        a = _timed(lambda: pcs.commit([(m, None)])[1].free(), warmup, reps)
        b = _timed(lambda: pcs.commit_quotient(chunks)[1].free(), warmup, reps)
        out.append("%-12s hiding commit (fill, randomize, LDE, salts, tree): %s" % (name, _fmt(a)))
        out.append("%-12s commit_quotient of %d chunks x %d (fill, inverse DFT, blind, LDE, salts, tree): %s" % (name, CHUNKS, _blind_width(w), _fmt(b)))
        if not plain:
            for what, nbytes in zip(("pcs_randomize_kernel", "pcs_blind_kernel"), hiding_bytes(log_h, w)):
                out.append("%-12s   %-22s %12d bytes read + written; a device-to-device copy of as many bytes (half read, half written) runs at %.0f GB/s"
                           % (name, what, nbytes, 2 * _copy_rate(nbytes // 2, warmup, reps)))
        pcs.free()
        del m, chunks


def fib_hiding_comparison(p3, warmup, reps, out):
    """the PCS calls of a hiding fib proof in the reference's configuration (Keccak, 2^19 rows; the quotient's values are given) beside
    FibAirProver(hiding=True).prove in the same process"""
    import torch
    log_n = 19
    pcs = p3.HidingFriPcs(p3.FriParameters(*FRI), "keccak")
    trace = p3.generate_trace_rows(0, 1, 1 << log_n)
    chunks = [torch.randint(0, P, (1 << log_n, 4), dtype=torch.int32, device="cuda") for _ in range(4)]
    rng = np.random.default_rng(2)
    z = [((rng.integers(0, P, 4, dtype=np.uint64) << 32) % P).astype(np.uint32) for _ in range(2)]

    def through():
        _, dt = pcs.commit([(trace, None)])
        _, dq = pcs.commit_quotient(chunks)
        _, dr = pcs.get_opt_randomization_poly_commitment(log_n)
        pcs.open([(dr, [[z[0]]]), (dt, [[z[0], z[1]]]), (dq, [[z[0]]] * 4)], p3.Challenger("keccak"))
        for d in (dt, dq, dr):
            d.free()
    a = _timed(through, warmup, reps)
    pr = p3.FibAirProver(log_n, params=p3.FriParameters(*FRI), hash="keccak", hiding=True)
    b = _timed(lambda: pr.prove(0, 1), warmup, reps)
    pr.close()
    out.append("hiding fib 2^19 Keccak through the PCS (3 commits + open, quotient values given): %s" % _fmt(a))
    out.append("hiding fib 2^19 Keccak FibAirProver(hiding=True).prove:                          %s" % _fmt(b))
    out.append("ratio of the medians (general path / hiding fib prover): %.2f" % (statistics.median(a) / statistics.median(b)))


def merge_hiding(prof_dir, out):
    """device times of the two kernels from a profiled --hiding --plain run: the dispatches in launch order are the shapes in
    HIDING_SHAPES order, (warm-up + reps) of each; the median per shape"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        out.append("no kernel trace under %s" % prof_dir)
        return
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    for kernel, which in (("pcs_randomize_kernel", 0), ("pcs_blind_kernel", 1)):
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        per = len(ns) // len(HIDING_SHAPES)
        for i, (log_h, w) in enumerate(HIDING_SHAPES):
            mine = ns[i * per:(i + 1) * per]
            if not mine:
                continue
            us, nbytes = statistics.median(mine) / 1e3, hiding_bytes(log_h, w)[which]
            out.append("2^%dx%-6d %-22s median %8.1f us of %d dispatches under rocprofv3 --kernel-trace; %d bytes -> %.0f GB/s"
                       % (log_h, _blind_width(w) if which else w, kernel, us, len(mine), nbytes, nbytes / (us * 1e3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--merge")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hiding", action="store_true")
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    a.output = a.output or os.path.join(ROOT, "profiles", "pcs_hiding_open_bench.txt" if a.hiding else "pcs_mixed_open_bench.txt" if a.mixed else "pcs_open_bench.txt")
    p3 = load_package()
    if a.mixed:
        out = ["# tools/pcs_bench.py --mixed: FRI parameters %s, Poseidon2 hashes, latency profile, 2 opening points on every matrix; device"
               % (FRI,), "# timestamps, %d warm-up and %d timed repetitions per figure" % (a.warmup, a.reps)]
        run_mixed(p3, a.warmup, a.reps, a.plain, out)
        if a.merge:
            merge_mixed(a.merge, out)
        text = "\n".join(out) + "\n"
        sys.stdout.write(text)
        if not a.plain:
            with open(a.output, "w") as f:
                f.write(text)
        return
    if a.hiding:
        out = ["# tools/pcs_bench.py --hiding: FRI parameters %s, %d random codewords, latency profile; device timestamps, %d warm-up and %d timed"
               % (FRI, NRC, a.warmup, a.reps), "# repetitions per figure"]
        run_hiding(p3, a.warmup, a.reps, a.plain, out)
        if not a.plain:
            fib_hiding_comparison(p3, a.warmup, a.reps, out)
        if a.merge:
            merge_hiding(a.merge, out)
        text = "\n".join(out) + "\n"
        sys.stdout.write(text)
        if not a.plain:
            with open(a.output, "w") as f:
                f.write(text)
        return
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
