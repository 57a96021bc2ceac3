"""Measurements of the bulk MMCS entries (p3hip_mmcs_open_batch_many_dev / p3hip_mmcs_verify_batch_many_dev); one JSON line per mode.

  throughput  verify_batch_many (per-lane form) of n = 2^20 and 2^22 openings of a 2^21 x 2 and a 2^20 x 8 tree, and, as the
              yardstick, commits of a 2^21-row and a 2^23-row matrix whose layers of 2^20 / 2^22 digests run the layer kernels
              (compress_layer_f64_kernel / keccak_compress_kernel) at the same lane counts.  Run it under
              `rocprofv3 --kernel-trace --output-format csv`; `summarize` turns the kernel trace into permutations/s.
  summarize   <kernel_trace.csv> <throughput JSON line file>: median kernel time per (kernel, grid), permutations/s, the ratio
  latency     one call of n openings on the 2^21 x 2 tree, per-lane and cooperative form alternated call by call in one process,
              medians of --reps calls (host wall time: enqueue + synchronise), n = 100 and a sweep up to where the medians cross
  open        100 single p3hip_mmcs_open_batch calls against one open_batch_many + one download, wall time, same tree
  oracle      the oracle's verify_batch over 2^16 openings on 16 host threads beside the device's time for the same openings
              (context, not credit)

Two measurements are recipes around this tool, not modes of it:
  bench A/B   `python bench.py --gpus 1 --steps 40 --warmup 2` in a checkout of the parent commit and in this tree, alternated three
              times in one session (the change touches no kernel a proof runs: the rates must agree within their spread)
  PMC         only if `summarize` shows a verify kernel below 0.9 of its yardstick: `rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES
              SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU --kernel-trace -- python tools/mmcs_verify_bench.py throughput --reps 1`, a run
              of its own (counters are never collected together with timing), read with tools/pmc_table.py

The permutation count of one opening is kept here: the absorb blocks of every height class + depth + injections.
Usage: python tools/mmcs_verify_bench.py MODE [--hash poseidon2|keccak] [--reps N]
Every GPU step of a session runs under `timeout -k 10 ...`, the steps chained with `&&`."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = 0x78000001
LANE, COOP = 1, 2


def _pkg():
    import __graft_entry__ as g
    p3 = g.load_package()
    ok, msg = p3.is_available()
    if not ok:
        raise SystemExit("no GPU: " + msg)  # a measurement without the device has no meaning: no fallback
    return p3


def perms_per_opening(dims, hash):
    """absorb blocks of every height class + depth + injections"""
    block = 34 if hash == "keccak" else 8
    maxh = max(h for h, _ in dims)
    depth = maxh.bit_length() - 1
    classes = {}
    for h, w in dims:
        classes[h] = classes.get(h, 0) + w
    absorb = sum(-(-w // block) for w in classes.values())
    return absorb + depth + (len(classes) - 1)


def _rand_dev(h, w, seed):
    import torch
    return torch.randint(0, P, (h, w), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


def _rand_idx(h, n, seed):
    import torch
    return torch.randint(0, h, (n,), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


def throughput(p3, a):
    import torch
    mm = p3.MerkleTreeMmcs(a.hash)
    out = {"mode": "throughput", "hash": a.hash, "reps": a.reps, "verify": [], "yardstick": []}
    for h, w in ((1 << 21, 2), (1 << 20, 8)):
        m = _rand_dev(h, w, h + w)
        root, tree = mm.commit([m])
        for n in (1 << 20, 1 << 22):
            idx = _rand_idx(h, n, n)
            rows, paths = mm.open_batch_many(idx, tree)
            for _ in range(1 + a.reps):
                st, rej = mm.verify_batch_many(root, [(h, w)], idx, rows, paths, form=LANE, with_rejected=True)
            torch.cuda.synchronize()
            assert int(p3.host_u32(rej)[0]) == 0
            out["verify"].append({"shape": [h, w], "n": n, "grid_threads": n, "perms_per_opening": perms_per_opening([(h, w)], a.hash),
                                  "kernel": "verify_lane_keccak_kernel" if a.hash == "keccak" else "verify_lane_p2_kernel"})
            del idx, rows, paths, st, rej
        tree.free()
        del m
    for h in (1 << 21, 1 << 23):  # the layer above the leaves has h / 2 digests: one permutation per lane, h / 2 lanes
        m = _rand_dev(h, 2, h)
        for _ in range(1 + a.reps):
            root, tree = mm.commit([m])
            tree.free()
        torch.cuda.synchronize()
        out["yardstick"].append({"rows": h, "grid_threads": h // 2, "perms": h // 2,
                                 "kernel": "keccak_compress_kernel" if a.hash == "keccak" else "compress_layer_f64_kernel"})
        del m
    return out


def summarize(a):
    """median duration per (kernel, grid) of a rocprofv3 kernel trace -> permutations/s and verify / yardstick ratios"""
    spec = [json.loads(l) for l in open(a.spec) if l.startswith("{")]
    spec = [s for s in spec if s.get("mode") == "throughput"][-1]
    durs = {}
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name")
            grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
            durs.setdefault((name.split("(")[0], grid), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))

    def med(kernel, grid):
        hit = [v for (nm, g), v in durs.items() if kernel in nm and g == grid]
        assert len(hit) == 1, (kernel, grid, [(k, len(v)) for k, v in durs.items() if kernel in k[0]])
        v = sorted(hit[0])[1:] if len(hit[0]) > 2 else hit[0]  # the first call of a kernel is unmeasured warm-up
        return statistics.median(v), len(v)

    out = {"mode": "summarize", "hash": spec["hash"], "yardstick": {}, "verify": []}
    for y in spec["yardstick"]:
        ns, calls = med(y["kernel"], y["grid_threads"])
        out["yardstick"][str(y["grid_threads"])] = {"kernel": y["kernel"], "median_us": round(ns / 1e3, 2), "calls": calls,
                                                    "gperms_per_s": round(y["perms"] / ns, 3)}
    for v in spec["verify"]:
        ns, calls = med(v["kernel"], v["grid_threads"])
        rate = v["n"] * v["perms_per_opening"] / ns
        out["verify"].append({"shape": v["shape"], "n": v["n"], "median_us": round(ns / 1e3, 2), "calls": calls,
                              "perms_per_opening": v["perms_per_opening"], "gperms_per_s": round(rate, 3),
                              "of_yardstick": round(rate / out["yardstick"][str(v["n"])]["gperms_per_s"], 3)})
    return out


def _time_forms(p3, kind, root, h, w, idx, rows, paths, reps):
    """the C call itself (every buffer allocated beforehand) + one stream synchronise, the two forms alternated call by call"""
    import ctypes as C
    import torch
    from plonky3_mobile_amd import _lib
    L = _lib.lib()
    n = idx.numel()
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    rej = torch.empty(1, dtype=torch.int32, device="cuda")
    hs, ws = (C.c_size_t * 1)(h), (C.c_size_t * 1)(w)
    vp = lambda t: C.c_void_p(t.data_ptr())
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (kind, root.ctypes.data_as(C.c_void_p), hs, ws, 1, vp(idx), n, vp(rows), vp(paths), vp(status), vp(rej), sp)

    def call(form):
        _lib.check(L.p3hip_mmcs_verify_batch_many_form_dev(form, *args))
        _lib.check(L.p3hip_sync(sp))
    t = {LANE: [], COOP: []}
    for form in (LANE, COOP):  # warm-up
        call(form)
        assert int(p3.host_u32(rej)[0]) == 0
    for _ in range(reps):
        for form in (LANE, COOP):
            t0 = time.perf_counter()
            call(form)
            t[form].append((time.perf_counter() - t0) * 1e6)
    return {k: (statistics.median(v), sorted(v)[len(v) // 10], sorted(v)[(9 * len(v)) // 10]) for k, v in t.items()}


def latency(p3, a):
    h, w = 1 << 21, 2
    out = {"mode": "latency", "shape": [h, w], "reps": a.reps, "profile": "latency (the forms are forced: the profile only moves the crossover)",
           "unit": "us: median, p10, p90 of host wall time of the C call + one synchronise", "hashes": {}}
    for hash, kind in (("poseidon2", 0), ("keccak", 1)):
        mm = p3.MerkleTreeMmcs(hash)
        m = _rand_dev(h, w, 3)
        root, tree = mm.commit([m])
        table = {}
        for n in (100, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
            idx = _rand_idx(h, n, n)
            rows, paths = mm.open_batch_many(idx, tree)
            r = _time_forms(p3, kind, root, h, w, idx, rows, paths, a.reps)
            table[str(n)] = {"lane": [round(x, 1) for x in r[LANE]], "coop": [round(x, 1) for x in r[COOP]]}
        tree.free()
        out["hashes"][hash] = table
    return out


def open_round_trips(p3, a):
    import torch
    h, w, n = 1 << 21, 2, 100
    out = {"mode": "open", "shape": [h, w], "n": n, "reps": a.reps, "unit": "ms, median of host wall time", "hashes": {}}
    for hash in ("poseidon2", "keccak"):
        mm = p3.MerkleTreeMmcs(hash)
        m = _rand_dev(h, w, 3)
        root, tree = mm.commit([m])
        idx = p3.host_u32(_rand_idx(h, n, 1))
        single, many = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            for i in idx:
                mm.open_batch(int(i), tree)
            t1 = time.perf_counter()
            rows, paths = mm.open_batch_many(idx, tree)
            hr, hp = p3.host_u32(rows), p3.host_u32(paths)
            t2 = time.perf_counter()
            if rep:
                single.append((t1 - t0) * 1e3)
                many.append((t2 - t1) * 1e3)
        tree.free()
        out["hashes"][hash] = {"100_single_calls_ms": round(statistics.median(single), 3), "one_bulk_call_and_download_ms": round(statistics.median(many), 3)}
    torch.cuda.synchronize()
    return out


def oracle_context(p3, a):
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from oracle import oracle as o
    o.build()
    h, w, n = 1 << 21, 2, 1 << 16
    out = {"mode": "oracle", "shape": [h, w], "n": n, "threads": 16, "hashes": {}}
    for hash, kind in (("poseidon2", 0), ("keccak", 1)):
        mm = p3.MerkleTreeMmcs(hash)
        m = _rand_dev(h, w, 3)
        root, tree = mm.commit([m])
        idx = _rand_idx(h, n, 2)
        rows, paths = mm.open_batch_many(idx, tree)
        mm.verify_batch_many(root, [(h, w)], idx, rows, paths)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = mm.verify_batch_many(root, [(h, w)], idx, rows, paths)
        torch.cuda.synchronize()
        dev_ms = (time.perf_counter() - t0) * 1e3
        assert not p3.host_u32(st).any()
        hi, hr, hp = p3.host_u32(idx), p3.host_u32(rows), p3.host_u32(paths)
        L = o.lib()
        hs, ws = (C.c_size_t * 1)(h), (C.c_size_t * 1)(w)
        depth = h.bit_length() - 1
        u32p = C.POINTER(C.c_uint32)

        def chunk(lo, hi_):
            bad = 0
            for i in range(lo, hi_):
                bad += L.p3o_mmcs_verify_batch_kind(C.c_int(kind), root.ctypes.data_as(u32p), hs, ws, C.c_size_t(1), C.c_size_t(int(hi[i])),
                                                    hr[i].ctypes.data_as(u32p), hp[i].ctypes.data_as(u32p), C.c_size_t(depth)) != 0
            return bad
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            bad = sum(ex.map(lambda k: chunk(k * n // 16, (k + 1) * n // 16), range(16)))
        host_ms = (time.perf_counter() - t0) * 1e3
        assert bad == 0
        tree.free()
        out["hashes"][hash] = {"device_call_ms": round(dev_ms, 3), "oracle_16_threads_ms": round(host_ms, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["throughput", "summarize", "latency", "open", "oracle"])
    ap.add_argument("--hash", default="poseidon2", choices=["poseidon2", "keccak"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace", help="summarize: the rocprofv3 kernel trace (csv)")
    ap.add_argument("--spec", help="summarize: the file holding the throughput mode's JSON line")
    a = ap.parse_args()
    if a.mode == "summarize":
        print(json.dumps(summarize(a)))
        return
    p3 = _pkg()
    print(json.dumps({"throughput": throughput, "latency": latency, "open": open_round_trips, "oracle": oracle_context}[a.mode](p3, a)))


if __name__ == "__main__":
    main()
