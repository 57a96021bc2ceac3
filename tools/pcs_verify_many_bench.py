#!/usr/bin/env python3
"""Host PCS verifier against the device batch verifier (PcsVerifier), on one box in one run, Poseidon2, FRI (1, 0, 100, 16):
  fib      the fib_air shape through the PCS: a 2-column trace at two slots and a 4-column quotient at one, 2^20 rows;
  w64      2^20 x 64 at one slot;
  w2633    2^16 x 2633 at two slots (5266 batched columns: the wave form of the reduced opening, the widest leaves);
  host     p3hip_pcs_verify, members/s on one thread and on 16 threads (the calls release the interpreter lock);
  device   PcsVerifier at n = 1, 8, 64, 512: HIP events around the launches of the device entry (members resident), and end to end
           through the host entry, the upload included;
  split    the device entry's kernels at n = 64 under rocprofv3 --kernel-trace --stats (a child process), when rocprofv3 is on the PATH.
Writes profiles/pcs_verify_many_bench.txt.      python3 tools/pcs_verify_many_bench.py [--out FILE] [--quick] [--shapes fib,w64,w2633]
  --mixed  the mixed-height verifier (PcsVerifier with a log height per matrix; proofs from TwoAdicFriPcs(mixed_heights=True); the host
           column is p3hip_pcs_verify_mixed) at n = 64 on two shapes, into profiles/pcs_verify_many_mixed_bench.txt:
           mixed  the fib-like shape with a second table eight times shorter: round 0 holds 2^20 x 2 and 2^17 x 2, both at two
                  slots, round 1 holds 2^20 x 4 at one;
           tall   the same with both tables at 2^20: what the shorter table saves and what its roll-in costs."""
import argparse
import csv
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

P = 0x78000001
HASH, FRI = "poseidon2", (1, 0, 100, 16)
# name -> (log_h, widths per round, slots per matrix per round)
SHAPES = {"fib": (20, [[2], [4]], [[[0, 1]], [[0]]]), "w64": (20, [[64]], [[[0]]]), "w2633": (16, [[2633]], [[[0, 1]]]),
          # log_h as per-matrix lists: the mixed entries
          "mixed": ([[20, 17], [20]], [[2, 2], [4]], [[[0, 1], [0, 1]], [[0]]]), "tall": ([[20, 20], [20]], [[2, 2], [4]], [[[0, 1], [0, 1]], [[0]]])}
MIXED_SHAPES = ("mixed", "tall")
DISTINCT = 4  # distinct members; larger batches repeat them (the verifier's work does not depend on which member it is)
FIB_DEVICE_MS_N64 = 0.559  # profiles/verify_many_bench.txt, cfg2, device n = 64


def monty(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def make_members(p3, name):
    """DISTINCT members of the shape, proved on the device: dicts of proof, roots, points, opened, state"""
    import torch
    log_h, widths, slots = SHAPES[name]
    rng = np.random.default_rng(len(name))
    n_slots = 1 + max(s for rs in slots for ms in rs for s in ms)
    lists = not isinstance(log_h, int)
    heights = log_h if lists else [[log_h] * len(ws) for ws in widths]
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*FRI), HASH, mixed_heights=lists)
    out = []
    for _ in range(DISTINCT):
        pts = monty(rng.integers(0, P, (n_slots, 4), dtype=np.uint64))
        rounds, roots = [], []
        for ws, ss, hs in zip(widths, slots, heights):
            mats = [(torch.randint(0, P, (1 << lh, w), dtype=torch.int32, device="cuda"), None) for w, lh in zip(ws, hs)]
            root, data = pcs.commit(mats)
            rounds.append((data, [[pts[s] for s in ms] for ms in ss]))
            roots.append(root)
        ch = p3.Challenger(HASH)
        ch.observe(monty(np.arange(1, 12)))
        state = ch.export_state()
        opened, proof = pcs.open(rounds, ch)
        out.append(dict(proof=proof, roots=np.stack(roots), points=pts, opened=opened.copy(), state=state))
        for d, _ in rounds:
            d.free()
    pcs.free()
    torch.cuda.empty_cache()
    return out


def verifier(p3, name, n):
    log_h, widths, slots = SHAPES[name]
    n_slots = 1 + max(s for rs in slots for ms in rs for s in ms)
    rounds = [[(w, sl) for w, sl in zip(ws, ss)] for ws, ss in zip(widths, slots)]
    return p3.PcsVerifier(log_h, rounds, n_slots, p3.FriParameters(*FRI), HASH, False, max_proofs=n)


def host_rate(p3, name, members, threads, seconds):
    lib = p3._lib.lib()
    log_h, widths, slots = SHAPES[name]
    fp = p3.FriParameters(*FRI)
    mats = (C.c_size_t * len(widths))(*[len(ws) for ws in widths])
    flat_w = [w for ws in widths for w in ws]
    cw = (C.c_size_t * len(flat_w))(*flat_w)
    counts = [len(ms) for ss in slots for ms in ss]
    cc = (C.c_size_t * len(counts))(*counts)
    lists = not isinstance(log_h, int)
    entry = lib.p3hip_pcs_verify_mixed if lists else lib.p3hip_pcs_verify
    if lists:
        flat_h = [lh for hs in log_h for lh in hs]
        log_h = (C.c_uint * len(flat_h))(*flat_h)
    prepared = []
    for m in members:
        pts = np.ascontiguousarray(np.concatenate([m["points"][s] for ss in slots for ms in ss for s in ms]))
        ch = p3.Challenger(HASH)
        ch.import_state(m["state"])
        prepared.append((np.ascontiguousarray(m["roots"]).reshape(-1), pts, np.ascontiguousarray(m["opened"]).reshape(-1),
                         (C.c_uint8 * len(m["proof"])).from_buffer_copy(m["proof"]), len(m["proof"]), ch))
    counts_done, stop = [0] * threads, time.perf_counter() + seconds

    def work(t):
        params = C.cast(fp._c(), C.c_void_p)
        k = t
        while time.perf_counter() < stop:
            roots, pts, opened, buf, ln, ch = prepared[k % len(prepared)]
            c, code = C.c_void_p(), C.c_int()
            assert lib.p3hip_challenger_clone(ch._h, C.byref(c)) == 0
            rc = entry(0, params, log_h, roots.ctypes.data_as(C.c_void_p), mats, cw, len(widths), cc, pts.ctypes.data_as(C.c_void_p),
                                      opened.ctypes.data_as(C.c_void_p), buf, ln, c, C.byref(code))
            lib.p3hip_challenger_destroy(c)
            assert rc == 0 and code.value == 0, (rc, code.value)
            counts_done[t] += 1
            k += 1

    t0 = time.perf_counter()
    ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return sum(counts_done) / (time.perf_counter() - t0)


def device_inputs(p3, torch, members, n):
    pick = [members[i % len(members)] for i in range(n)]
    plen = len(members[0]["proof"])
    host = np.empty((n, plen), dtype=np.uint8)
    for i, m in enumerate(pick):
        host[i] = np.frombuffer(m["proof"], dtype=np.uint8)
    return [torch.from_numpy(host).cuda()] + [p3.dev_u32(np.stack([m[k] for m in pick])) for k in ("roots", "points", "opened", "state")]


def device_rates(p3, name, members, n, reps):
    import torch
    ver = verifier(p3, name, n)
    try:
        args = device_inputs(p3, torch, members, n)
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        rejected = torch.empty(1, dtype=torch.int32, device="cuda")
        out = torch.empty((n, p3.pcs.STATE_WORDS), dtype=torch.int32, device="cuda")
        for _ in range(2):
            ver.verify_many_dev(*args, n=n, status=status, rejected=rejected, chal_out=out)
        torch.cuda.synchronize()
        assert int(rejected.cpu()[0]) == 0
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ver.verify_many_dev(*args, n=n, status=status, rejected=rejected, chal_out=out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        dev_ms = ms[len(ms) // 2]
        del args
        pick = [members[i % len(members)] for i in range(n)]
        hargs = ([m["proof"] for m in pick], np.stack([m["roots"] for m in pick]), np.stack([m["points"] for m in pick]),
                 np.stack([m["opened"] for m in pick]))

        def chals():
            cs = []
            for m in pick:
                c = p3.Challenger(HASH)
                c.import_state(m["state"])
                cs.append(c)
            return cs
        assert not ver.verify_many(*hargs, chals()).any()  # the first call allocates the staging
        e2e = []
        for _ in range(max(2, reps // 2)):
            cs = chals()
            t0 = time.perf_counter()
            ver.verify_many(*hargs, cs)
            e2e.append(time.perf_counter() - t0)
        e2e.sort()
        return dev_ms, e2e[len(e2e) // 2] * 1e3, ver.wave_form
    finally:
        ver.close()


def trace_workload(p3, name, n):
    """the child under rocprofv3: the device entry alone, ten calls"""
    import torch
    members = make_members(p3, name)
    ver = verifier(p3, name, n)
    args = device_inputs(p3, torch, members, n)
    for _ in range(10):
        ver.verify_many_dev(*args, n=n)
    torch.cuda.synchronize()
    ver.close()


def kernel_split(name, n):
    """-> (lines, {kernel: average us})"""
    if not shutil.which("rocprofv3"):
        return ["  (rocprofv3 is not on the PATH: no per-kernel split)"], {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "pvm", "--", sys.executable,
               os.path.abspath(__file__), "--trace-workload", name, "--trace-n", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=500)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return ["  (the traced child failed: rc %d)" % r.returncode], {}
        rows = [row for row in csv.DictReader(open(files[0])) if "pv_" in row["Name"]]
    out, avg = [], {}
    for row in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        kname = row["Name"].replace("void ", "").replace("p3::(anonymous namespace)::", "").split("(")[0]
        avg[kname] = float(row["AverageNs"]) / 1e3
        out.append("  %-44s calls %3s  avg %10.1f us  min %10.1f us  max %10.1f us" % (kname, row["Calls"], float(row["AverageNs"]) / 1e3,
                                                                                     float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))
    return out, avg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--mixed", action="store_true", help="the mixed-height shapes at n = 64")
    ap.add_argument("--quick", action="store_true", help="n = 1, 8, 64 only and shorter host timing")
    ap.add_argument("--shapes")
    ap.add_argument("--trace-workload")
    ap.add_argument("--trace-n", type=int, default=64)
    a = ap.parse_args()
    p3 = load_package()
    if a.trace_workload:
        trace_workload(p3, a.trace_workload, a.trace_n)
        return
    if not a.out:
        a.out = os.path.join(ROOT, "profiles", "pcs_verify_many_mixed_bench.txt" if a.mixed else "pcs_verify_many_bench.txt")
    if not a.shapes:
        a.shapes = ",".join(MIXED_SHAPES if a.mixed else [s for s in SHAPES if s not in MIXED_SHAPES])
    names = [s for s in a.shapes.split(",") if s]
    lines = ["# tools/pcs_verify_many_bench.py: host PCS verifier against the device batch verifier, one box, one run.",
             "# %s, FRI (log_blowup, log_final_poly_len, queries, pow bits) = %s; host threads are Python threads around the C entry" % (HASH, FRI,),
             "# (the interpreter lock is released for the call).  device = HIP events around the device entry's launches, members resident;",
             "# e2e = the host entry: upload + verify + download, wall clock.  Medians."]
    if a.mixed:
        lines.append("# --mixed: a log height per matrix (p3hip_pcs_verifier_create_mixed); the host verifier is p3hip_pcs_verify_mixed.")
    splits = {name: kernel_split(name, 64) for name in names}  # the traced children first: this process has not opened the GPU yet
    verdict = []
    for name in names:
        log_h, widths, slots = SHAPES[name]
        members = make_members(p3, name)
        secs = 2.0 if a.quick else 4.0
        h1 = host_rate(p3, name, members, 1, secs)
        h16 = host_rate(p3, name, members, 16, secs)
        total = sum(w * len(ms) for ws, ss in zip(widths, slots) for w, ms in zip(ws, ss))
        lines += ["", "%s: 2^%s rows, widths %s, %d batched columns, proof %d bytes" % (name, log_h, widths, total, len(members[0]["proof"])),
                  "  host verifier    1 thread  %9.1f members/s  (%.2f ms per member)" % (h1, 1e3 / h1),
                  "  host verifier   16 threads %9.1f members/s" % h16]
        for n in (64,) if a.mixed else (1, 8, 64) if a.quick else (1, 8, 64, 512):
            dev_ms, e2e_ms, wave = device_rates(p3, name, members, n, 10 if n < 512 else 6)
            lines.append("  device n = %-4d  device %9.3f ms = %9.1f members/s    e2e %9.3f ms = %9.1f members/s" %
                         (n, dev_ms, n / dev_ms * 1e3, e2e_ms, n / e2e_ms * 1e3))
            if n == 64:
                verdict.append("%s, n = 64: device-resident %.1f members/s against %.1f on 16 host threads: %s" %
                               (name, n / dev_ms * 1e3, h16, "the device form wins" if n / dev_ms * 1e3 > h16 else "THE DEVICE FORM LOSES"))
                if name == "fib":
                    verdict.append("fib, n = 64: %.3f ms against the fib_air device verifier's %.3f ms (profiles/verify_many_bench.txt): ratio %.2f" %
                                   (dev_ms, FIB_DEVICE_MS_N64, dev_ms / FIB_DEVICE_MS_N64))
        lines.append("  reduced opening: %s form" % ("wave" if wave else "lane"))
        lines.append("  kernels of one device call at n = 64 (rocprofv3 --kernel-trace --stats, ten calls):")
        lines += splits[name][0]
    lines += [""] + verdict
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
