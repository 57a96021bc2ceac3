#!/usr/bin/env python3
"""The device batch verifier of caller-defined AIRs (AirVerifier) against a loop of the host verifier p3hip_air_verify, on one box in
one run: 64 proofs of the fib AIR and 64 of the test AIR (C) (width 70, degree 4, 770 instructions) at log_n 10, Poseidon2, proved by
prove_air.
  device   HIP events around the launches of verify_many_dev, members resident: the median of 13;
  host     the same 64 members through Air.verify one after the other, wall clock: the median of 13;
  split    the kernels of the device entry under rocprofv3 --kernel-trace --stats (a child process, a run of its own), the two new
           ones (av_transcript_kernel, av_eval_kernel) among them, when rocprofv3 is on the PATH.
Writes profiles/air_verify_many.txt.      python3 tools/air_verify_bench.py [--out FILE]"""
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

HASH, LOG_N, N, REPS = "poseidon2", 10, 64, 13
FRI = {"fib": (1, 0, 100, 16), "C": (2, 0, 100, 16)}  # (C) has four quotient chunks (log_quotient_degree 2): log_blowup 2
DISTINCT = 4  # distinct members; the batch repeats them (the verifier's work does not depend on which member it is)


def make_members(p3, name):
    """-> (air, [(proof, public values)]) proved on the device"""
    import air_ref as A
    air, gen = A.all_airs(p3)[name]
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*FRI[name]), HASH)
    out = []
    for k in range(DISTINCT):
        trace, pis = gen(LOG_N, **({"a": k, "b": k + 1} if name == "fib" else {"s": 9 + k}))
        out.append((p3.prove_air(air, pcs, p3.dev_u32(trace), pis), pis))
    pcs.free()
    return air, out


def device_inputs(p3, members):
    import torch
    pick = [members[i % len(members)] for i in range(N)]
    host = np.stack([np.frombuffer(pr, dtype=np.uint8) for pr, _ in pick])
    return torch.from_numpy(host).cuda(), p3.dev_u32(np.stack([pi for _, pi in pick])), pick


def measure(p3, name):
    import torch
    air, members = make_members(p3, name)
    fp = p3.FriParameters(*FRI[name])
    ver = p3.AirVerifier(air, LOG_N, fp, HASH, max_proofs=N)
    proofs, pis, pick = device_inputs(p3, members)
    status = torch.empty(N, dtype=torch.int32, device="cuda")
    rejected = torch.empty(1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        ver.verify_many_dev(proofs, pis, n=N, status=status, rejected=rejected)
    torch.cuda.synchronize()
    assert int(rejected.cpu()[0]) == 0
    dev = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ver.verify_many_dev(proofs, pis, n=N, status=status, rejected=rejected)
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1))
    host = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for pr, pi in pick:
            assert air.verify(pr, pi, LOG_N, fp, HASH) == 0
        host.append((time.perf_counter() - t0) * 1e3)
    ver.close()
    return sorted(dev)[REPS // 2], sorted(host)[REPS // 2], len(members[0][0]), air


def trace_workload(p3, name):
    """the child under rocprofv3: the device entry alone, thirteen calls"""
    import torch
    air, members = make_members(p3, name)
    ver = p3.AirVerifier(air, LOG_N, p3.FriParameters(*FRI[name]), HASH, max_proofs=N)
    proofs, pis, _ = device_inputs(p3, members)
    for _ in range(REPS):
        ver.verify_many_dev(proofs, pis, n=N)
    torch.cuda.synchronize()
    ver.close()


def kernel_split(name):
    if not shutil.which("rocprofv3"):
        return ["  (rocprofv3 is not on the PATH: no per-kernel split)"]
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "avm", "--", sys.executable, os.path.abspath(__file__),
               "--trace-workload", name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=500)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return ["  (the traced child failed: rc %d)" % r.returncode]
        rows = [row for row in csv.DictReader(open(files[0])) if "av_" in row["Name"] or "pv_" in row["Name"]]
    out = []
    for row in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        kname = row["Name"].replace("void ", "").replace("p3::(anonymous namespace)::", "").split("(")[0]
        out.append("  %-44s calls %3s  avg %10.1f us  min %10.1f us  max %10.1f us" % (kname, row["Calls"], float(row["AverageNs"]) / 1e3,
                                                                                     float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_verify_many.txt"))
    ap.add_argument("--trace-workload")
    a = ap.parse_args()
    p3 = load_package()
    if a.trace_workload:
        trace_workload(p3, a.trace_workload)
        return
    lines = ["# tools/air_verify_bench.py: the device batch verifier of caller-defined AIRs against a loop of the host verifier, one box, one run.",
             "# %s, log_n %d, %d members (%d distinct, repeated), medians of %d.  device = HIP events around the launches of verify_many_dev," % (HASH, LOG_N, N, DISTINCT, REPS),
             "# members resident; host = %d calls of p3hip_air_verify one after the other on one thread, wall clock." % N]
    splits = {name: kernel_split(name) for name in FRI}  # the traced children first: this process has not opened the GPU yet
    for name in FRI:
        dev_ms, host_ms, plen, air = measure(p3, name)
        lines += ["", "%s: width %d, %d instructions, %d constraints, %d chunk(s), FRI %s, proof %d bytes" %
                  (name, air.width, air.n_instructions, air.n_constraints, air.n_chunks, FRI[name], plen),
                  "  device  %9.3f ms = %9.1f members/s" % (dev_ms, N / dev_ms * 1e3),
                  "  host    %9.3f ms = %9.1f members/s   (device / host time: %.3f)" % (host_ms, N / host_ms * 1e3, dev_ms / host_ms),
                  "  kernels of one device call (rocprofv3 --kernel-trace --stats, %d calls):" % REPS] + splits[name]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
