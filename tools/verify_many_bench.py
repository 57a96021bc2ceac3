#!/usr/bin/env python3
"""Host verifier against the device batch verifier, on one box in one run, at cfg2 (Poseidon2, 2^20 rows, blowup 2, 100 queries, 16
proof-of-work bits) and at the reference's configuration at that size (Keccak + hiding):
  host    p3hip_verify_fib_air_hash / _hiding, proofs/s on one thread and on 16 threads (the calls release the interpreter lock);
  device  FibAirVerifier at n = 1, 8, 64, 512: HIP events around the launches of the device entry (proofs resident), and end to end
          through the host entry, the upload included;
  split   the device entry's kernels (the front kernel and the owned PCS verifier's) at n = 64 under rocprofv3 --kernel-trace --stats (a child process), when rocprofv3 is on the PATH.
Writes profiles/verify_many_bench.txt.      python3 tools/verify_many_bench.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

P = 0x78000001
CONFIGS = {"cfg2": ("poseidon2", False), "cfg2_keccak_hiding": ("keccak", True)}
LOG_N, FRI = 20, (1, 0, 100, 16)
KERNELS = ("fv_", "pv_")  # the device entry's kernels: the fib front kernel and the owned PCS verifier's four
DISTINCT = 8  # distinct proofs; larger batches repeat them (the verifier's work does not depend on which proof it is)


def monty(v):
    return ((v % P) << 32) % P


def make_proofs(p3, hash_name, hiding):
    pool = p3.FibAirBatchProver(LOG_N, n_provers=2, params=p3.FriParameters(*FRI), hash=hash_name, hiding=hiding, seed=1)
    insts = [(k, k + 1) for k in range(DISTINCT)]
    try:
        proofs = pool.prove(insts)
    finally:
        pool.close()
    return proofs, [(a, b, p3.fib_public_x(a, b, 1 << LOG_N)) for a, b in insts]


def host_rate(p3, proofs, insts, hash_name, hiding, threads, seconds):
    lib = p3._lib.lib()
    fn = lib.p3hip_verify_fib_air_hiding if hiding else lib.p3hip_verify_fib_air_hash
    fp = p3.FriParameters(*FRI)
    bufs = [(C.c_uint8 * len(p)).from_buffer_copy(p) for p in proofs]
    counts, stop = [0] * threads, time.perf_counter() + seconds

    def work(t):
        params = C.cast(fp._c(), C.c_void_p)
        k = t
        while time.perf_counter() < stop:
            i = k % len(proofs)
            rc = fn(0 if hash_name == "poseidon2" else 1, bufs[i], len(proofs[i]), insts[i][0], insts[i][1], insts[i][2], LOG_N, params)
            assert rc == 0, rc
            counts[t] += 1
            k += 1

    t0 = time.perf_counter()
    ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return sum(counts) / (time.perf_counter() - t0)


def device_inputs(torch, proofs, insts, n):
    import numpy as np
    plen = len(proofs[0])
    host = np.empty((n, plen), dtype=np.uint8)
    for i in range(n):
        host[i] = np.frombuffer(proofs[i % len(proofs)], dtype=np.uint8)
    pis = np.array([[monty(v) for v in insts[i % len(insts)]] for i in range(n)], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(host).cuda(), torch.from_numpy(pis).cuda()


def device_rates(p3, proofs, insts, hash_name, hiding, n, reps):
    import torch
    ver = p3.FibAirVerifier(LOG_N, p3.FriParameters(*FRI), hash_name, hiding, max_proofs=n)
    try:
        d_proofs, d_pis = device_inputs(torch, proofs, insts, n)
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        rejected = torch.empty(1, dtype=torch.int32, device="cuda")
        for _ in range(2):
            ver.verify_many_dev(d_proofs, d_pis, None, status, rejected, n=n)
        torch.cuda.synchronize()
        assert int(rejected.cpu()[0]) == 0
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ver.verify_many_dev(d_proofs, d_pis, None, status, rejected, n=n)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        dev_ms = ms[len(ms) // 2]
        del d_proofs
        plist = [proofs[i % len(proofs)] for i in range(n)]
        ilist = [insts[i % len(insts)] for i in range(n)]
        assert not ver.verify_many(plist, ilist).any()  # the first call allocates the staging
        e2e = []
        for _ in range(max(2, reps // 2)):
            t0 = time.perf_counter()
            ver.verify_many(plist, ilist)
            e2e.append(time.perf_counter() - t0)
        e2e.sort()
        return dev_ms, e2e[len(e2e) // 2] * 1e3
    finally:
        ver.close()


def trace_workload(p3, name, n):
    """the child under rocprofv3: the device entry alone, ten calls"""
    import torch
    hash_name, hiding = CONFIGS[name]
    proofs, insts = make_proofs(p3, hash_name, hiding)
    ver = p3.FibAirVerifier(LOG_N, p3.FriParameters(*FRI), hash_name, hiding, max_proofs=n)
    d_proofs, d_pis = device_inputs(torch, proofs, insts, n)
    for _ in range(10):
        ver.verify_many_dev(d_proofs, d_pis, None, n=n)
    torch.cuda.synchronize()
    ver.close()


def kernel_split(name, n):
    if not shutil.which("rocprofv3"):
        return ["  (rocprofv3 is not on the PATH: no per-kernel split)"]
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "vm", "--", sys.executable,
               os.path.abspath(__file__), "--trace-workload", name, "--trace-n", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return ["  (the traced child failed: rc %d)" % r.returncode]
        rows = [row for row in csv.DictReader(open(files[0])) if any(k in row["Name"] for k in KERNELS)]
    out = []
    for row in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        kname = row["Name"].replace("void ", "").replace("p3::(anonymous namespace)::", "").split("(")[0]
        out.append("  %-44s calls %3s  avg %10.1f us  min %10.1f us  max %10.1f us" % (kname, row["Calls"], float(row["AverageNs"]) / 1e3,
                                                                                     float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_many_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 1, 8, 64 only and shorter host timing")
    ap.add_argument("--trace-workload")
    ap.add_argument("--trace-n", type=int, default=64)
    a = ap.parse_args()
    p3 = load_package()
    if a.trace_workload:
        trace_workload(p3, a.trace_workload, a.trace_n)
        return
    lines = ["# tools/verify_many_bench.py: host verifier against the device batch verifier, one box, one run.",
             "# 2^%d rows, FRI (log_blowup, log_final_poly_len, queries, pow bits) = %s; host threads are Python threads around the C entry" % (LOG_N, FRI,),
             "# (the interpreter lock is released for the call).  device = HIP events around the device entry's launches, proofs resident;",
             "# e2e = the host entry: upload + verify + download, wall clock.  Medians."]
    splits = {name: kernel_split(name, 64) for name in CONFIGS}  # the traced children first: this process has not opened the GPU yet
    verdict = []
    for name, (hash_name, hiding) in CONFIGS.items():
        proofs, insts = make_proofs(p3, hash_name, hiding)
        secs = 2.0 if a.quick else 4.0
        h1 = host_rate(p3, proofs, insts, hash_name, hiding, 1, secs)
        h16 = host_rate(p3, proofs, insts, hash_name, hiding, 16, secs)
        lines += ["", "%s (%s%s), proof %d bytes" % (name, hash_name, ", hiding" if hiding else "", len(proofs[0])),
                  "  host verifier    1 thread  %9.1f proofs/s  (%.2f ms per proof)" % (h1, 1e3 / h1),
                  "  host verifier   16 threads %9.1f proofs/s" % h16]
        for n in (1, 8, 64) if a.quick else (1, 8, 64, 512):
            dev_ms, e2e_ms = device_rates(p3, proofs, insts, hash_name, hiding, n, 10 if n < 512 else 6)
            lines.append("  device n = %-4d  device %9.3f ms = %9.1f proofs/s    e2e %9.3f ms = %9.1f proofs/s" %
                         (n, dev_ms, n / dev_ms * 1e3, e2e_ms, n / e2e_ms * 1e3))
            if n == 64:
                verdict.append("%s, n = 64: device-resident %.1f proofs/s against %.1f on 16 host threads: %s" %
                               (name, n / dev_ms * 1e3, h16, "the device form wins" if n / dev_ms * 1e3 > h16 else "THE DEVICE FORM LOSES"))
        lines.append("  kernels of one device call at n = 64 (rocprofv3 --kernel-trace --stats, ten calls):")
        lines += splits[name]
    lines += [""] + verdict
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
