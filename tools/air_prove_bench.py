#!/usr/bin/env python3
"""AirProver (one device-resident launch chain, one synchronisation) against prove_air (the host drives the challenger: two commits and
an open, three synchronisations) and, for the fib program, against FibAirProver.prove_trace (the dedicated kernels), on one box in one
process, latency profile, Poseidon2, FRI (log_blowup, 0, 100, 16).
  wall     time.perf_counter around ONE proof of a device-resident trace, the device idle before and the proof's bytes in host memory
           after; the two sides alternate, the median of 13 after two proofs of warm-up each.
  launches kernel dispatches of one AirProver proof: rocprofv3 --kernel-trace over a child that proves once and over one that proves
           three times, the difference halved (first-use table builds drop out), when rocprofv3 is on the PATH.
The (C) trace is random words: neither prover judges the trace and the work does not depend on its values.
Writes profiles/air_prove_bench.txt.      python3 tools/air_prove_bench.py [--out FILE]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402

HASH, REPS, WARM = "poseidon2", 13, 2
CASES = [("fib", 10), ("fib", 16), ("fib", 20), ("C", 16)]
P = 0x78000001


def instance(p3, name, log_n):
    """-> (air, device trace, public values, FRI parameters, canonical fib publics or None)"""
    import air_ref as A
    air = A.all_airs(p3)[name][0]
    fp = p3.FriParameters(max(1, air.log_quotient_degree), 0, 100, 16)
    if name == "fib":
        x = p3.fib_public_x(0, 1, 1 << log_n)
        pis = np.array([p3.air.to_monty(v) for v in (0, 1, x)], dtype=np.uint32)
        return air, p3.generate_trace_rows(0, 1, 1 << log_n), pis, fp, [0, 1, x]
    rng = np.random.default_rng(16)
    trace = rng.integers(0, P, (1 << log_n, air.width), dtype=np.uint64).astype(np.uint32)
    return air, p3.dev_u32(trace), rng.integers(0, P, air.n_public, dtype=np.uint64).astype(np.uint32), fp, None


def median_ms(sides):
    """sides: callables, each one proof; alternated; -> the median wall time of each in ms, and the last result of each"""
    import torch
    times, last = [[] for _ in sides], [None] * len(sides)
    for r in range(WARM + REPS):
        for i, f in enumerate(sides):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[i] = f()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[i].append(dt)
    return [sorted(t)[REPS // 2] for t in times], last


def measure(p3, name, log_n):
    air, trace, pis, fp, fib_pis = instance(p3, name, log_n)
    pr = p3.AirProver(air, log_n, fp, HASH, "latency")
    pcs = p3.TwoAdicFriPcs(fp, HASH)
    sides = [lambda: pr.prove(trace, pis), lambda: p3.prove_air(air, pcs, trace, pis)]
    fib = None
    if fib_pis is not None and log_n == 20:
        fib = p3.FibAirProver(log_n, params=fp, hash=HASH)
        sides.append(lambda: fib.prove_trace(trace, fib_pis))
    ms, proofs = median_ms(sides)
    assert all(p == proofs[0] for p in proofs), "the sides' bytes differ"
    pr.close()
    pcs.free()
    if fib:
        fib.close()
    return air, ms, len(proofs[0])


def trace_workload(p3, n_proofs):
    """the child under rocprofv3: fib at 2^16, n_proofs proofs of AirProver"""
    import torch
    air, trace, pis, fp, _ = instance(p3, "fib", 16)
    pr = p3.AirProver(air, 16, fp, HASH, "latency")
    torch.cuda.synchronize()
    for _ in range(n_proofs):
        pr.prove(trace, pis)
    pr.close()


def dispatches(n_proofs):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "apb", "--", sys.executable, os.path.abspath(__file__),
               "--trace-workload", str(n_proofs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None
        rows = list(csv.DictReader(open(files[0])))
        return len([row for row in rows if "generate_trace" not in row.get("Kernel_Name", "")])


def launch_count():
    if not shutil.which("rocprofv3"):
        return "launches of one AirProver proof: not measured (rocprofv3 is not on the PATH)"
    one, three = dispatches(1), dispatches(3)
    if one is None or three is None:
        return "launches of one AirProver proof: not measured (the traced child failed)"
    return "launches of one AirProver proof, fib at 2^16 (rocprofv3 --kernel-trace, a run of its own): %d  (%d dispatches with one proof, %d with three)" % (
        (three - one) // 2, one, three)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_prove_bench.txt"))
    ap.add_argument("--trace-workload", type=int)
    a = ap.parse_args()
    p3 = load_package()
    if a.trace_workload:
        trace_workload(p3, a.trace_workload)
        return
    launches = launch_count()  # the traced children first: this process has not opened the GPU yet
    lines = ["# tools/air_prove_bench.py: AirProver.prove against prove_air (the baseline), one box, one process, latency profile, %s." % HASH,
             "# Wall time of one proof of a device-resident trace, the sides alternating, medians of %d after %d warm-up proofs each." % (REPS, WARM),
             "# libp3hip.so sha256 %s" % p3._lib.lib_sha256(), "# sources   sha256 %s" % p3._lib.src_sha256(), ""]
    for name, log_n in CASES:
        air, ms, plen = measure(p3, name, log_n)
        lines.append("%-3s 2^%-2d  width %2d, %3d constraints, %d chunk(s), proof %d bytes:  AirProver %9.3f ms   prove_air %9.3f ms   (AirProver / prove_air %.3f)" %
                     (name, log_n, air.width, air.n_constraints, air.n_chunks, plen, ms[0], ms[1], ms[0] / ms[1]))
        if len(ms) == 3:
            lines.append("           FibAirProver.prove_trace %9.3f ms   (AirProver / FibAirProver %.3f: the interpreter and the in-lane selectors)" % (ms[2], ms[0] / ms[2]))
    lines += ["", launches]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
