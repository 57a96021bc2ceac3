"""Measurements of the caller-trace entries (include/p3hip.h "a CALLER's trace"); one JSON line per mode on stdout.

  latency  a lone 2^20 proof, latency profile, the bench's FRI parameters: prove(a, b) against prove_trace on a device trace and
           on a host trace (the upload into the arena is the difference), alternated proof by proof, medians of --reps each
  check    check_fib_trace over 2^20 and 2^24 Fibonacci traces, --reps times each (run under
           `rocprofv3 --kernel-trace --stats` for the kernel's time; the HBM fraction is 8 n bytes / time / 8 TB/s)
  tiny     the reference's n = 8 Keccak hiding instance through prove_trace on a device trace, --reps times (under
           `rocprofv3 --kernel-trace` each proof must be ONE kernel launch)

Usage: python tools/prove_trace_bench.py {latency|check|tiny} [--reps N]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E spec


def _pkg():
    import __graft_entry__ as g
    p3 = g.load_package()
    ok, msg = p3.is_available()
    if not ok:
        raise SystemExit("no GPU: " + msg)  # a measurement without the device has no meaning: no fallback
    return p3


def _x(p3, trace):
    """the last row's right value as a canonical int (the public value x)"""
    w = int(p3.host_u32(trace[-1:, 1:])[0, 0])
    return (w * pow(1 << 32, -1, p3.P)) % p3.P


def latency(p3, reps):
    import torch
    log_n = 20
    fp = p3.FriParameters(1, 0, 100, 16)
    pr = p3.FibAirProver(log_n, params=fp)
    trace = p3.generate_trace_rows(0, 1, 1 << log_n)
    torch.cuda.synchronize()
    pis = [0, 1, _x(p3, trace)]
    host = p3.host_u32(trace).copy()
    ref = pr.prove(0, 1)
    assert pr.prove_trace(trace, pis) == ref and pr.prove_trace(host, pis) == ref, "bytes differ"
    t = {"prove_ab": [], "prove_trace_dev": [], "prove_trace_host": []}
    for _ in range(3):  # warm-up
        pr.prove(0, 1); pr.prove_trace(trace, pis); pr.prove_trace(host, pis)
    for _ in range(reps):
        for k, f in (("prove_ab", lambda: pr.prove(0, 1)), ("prove_trace_dev", lambda: pr.prove_trace(trace, pis)),
                     ("prove_trace_host", lambda: pr.prove_trace(host, pis))):
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    pr.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"mode": "latency", "log_n": log_n, "fri": [1, 0, 100, 16], "profile": "latency", "reps": reps,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "p10_p90_ms": {k: [round(sorted(v)[len(v) // 10], 4), round(sorted(v)[(9 * len(v)) // 10], 4)] for k, v in t.items()},
            "trace_dev_vs_ab": round(med["prove_trace_dev"] / med["prove_ab"] - 1, 4),
            "host_upload_added_ms": round(med["prove_trace_host"] - med["prove_trace_dev"], 4),
            "host_upload_bytes": 8 << log_n}


def check(p3, reps):
    import torch
    out = {"mode": "check", "reps": reps, "sizes": {}}
    for log_n in (20, 24):
        n = 1 << log_n
        trace = p3.generate_trace_rows(0, 1, n)
        torch.cuda.synchronize()
        pis = [0, 1, _x(p3, trace)]
        assert p3.check_fib_trace(trace, pis) == (None, 0, 0)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            p3.check_fib_trace(trace, pis)  # synchronises: host wall time of one call (launch + kernel + 16-byte copy)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["sizes"][str(log_n)] = {"bytes": 8 * n, "call_median_ms": round(statistics.median(ts), 4),
                                    "kernel_time_for_half_peak_us": round(8 * n / (HBM_PEAK / 2) * 1e6, 2)}
    return out


def tiny(p3, reps):
    import torch
    fp = p3.FriParameters(2, 2, 2, 1)
    pr = p3.FibAirProver(3, params=fp, hash="keccak", hiding=True, seed=1)
    trace = p3.generate_trace_rows(0, 1, 8)
    torch.cuda.synchronize()
    ref = pr.prove(0, 1)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert pr.prove_trace(trace, [0, 1, 21]) == ref
        ts.append((time.perf_counter() - t0) * 1e3)
    pr.close()
    return {"mode": "tiny", "reps": reps, "proofs_of_prove_trace": reps, "call_median_ms": round(statistics.median(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["latency", "check", "tiny"])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    p3 = _pkg()
    print(json.dumps({"latency": latency, "check": check, "tiny": tiny}[a.mode](p3, a.reps)))


if __name__ == "__main__":
    main()
