"""Child process of tests/test_gpu_collectives.py (not a test module): opens a world-size-1 process group and drives
plonky3_mobile_amd.batch on the branch its --device selects ("cuda": RCCL, device staging, pinned landings and events; "cpu":
gloo on host tensors, the control).  It writes what it gathered to a pickle; the parent compares that with the oracle.

  python tests/_collectives_child.py --backend nccl --device cuda --out FILE [--part all|pipelined] [--flip STEP:INSTANCE:OFFSET]

MASTER_PORT comes from the parent.  --flip (negative control): after the sink has written instance INSTANCE of step STEP and
before that step's gather is launched, the byte at OFFSET of its proof is inverted in the pinned host staging row."""
import argparse
import ctypes
import os
import pickle
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOG_N, BATCH, THREADS, STEPS = 10, 7, 3, 7  # bench's form at 2^10: 7 steps, so every staging slot is used more than once


class _DirectSink:
    """The direct sink form (a restatement of bench.py's): the prover writes each proof into its staging row itself."""
    direct = True

    def __init__(self, put, rows):
        self.put, self.rows = put, rows

    def buffer(self, i):
        return self.put.row_ptr(self.rows[i])

    def done(self, i, length):
        self.put.set(self.rows[i], i, length)


def pipelined(p3, batch, device, flip):
    """bench.py's loop with a real FibAirJob: one DescriptorScatter run for every step, a ProofGatherer allocated before the loop,
    issue(k + 1) before retire(k), the bytes sink on even steps and the direct sink on odd ones, rank 0 reading views."""
    from plonky3_mobile_amd import bench_support as bs
    job = bs.FibAirJob(p3, LOG_N, 1, BATCH, threads=THREADS)
    width = len(job.prove_one(0, 1))
    g = batch.ProofGatherer(BATCH, device, width=width)
    steps = [[(k * BATCH + i, k * BATCH + i + 1) for i in range(BATCH)] for k in range(STEPS)]
    pend = batch.DescriptorScatter(STEPS, BATCH, device).run(steps)
    out = {"width": width, "descriptors": {}, "proofs": {}, "views_after_next": {}}
    views, pending = {}, [None]

    def issue(k):
        mine = pend.step(k)
        out["descriptors"][k] = mine
        rows = {i: r for r, (i, _, _) in enumerate(mine)}
        put, slot = g.open(len(mine), width)
        sink = _DirectSink(put, rows) if k % 2 else (lambda i, pf: put(rows[i], i, pf))
        job.step_begin([(i, a) for i, a, _ in mine], sink)
        return k, rows, slot

    def collect(k, res):
        views[k] = res
        out["proofs"][k] = [bytes(v) for v in res]
        if k - 1 in views:  # step k - 1's views, kept while step k was gathered and collected
            out["views_after_next"][k - 1] = [bytes(v) for v in views.pop(k - 1)]

    def retire(k, rows, slot):
        job.step_end()
        if flip is not None and flip[0] == k:
            row = slot["h"].numpy()[rows[flip[1]]]
            row[batch.ROW_HEADER + flip[2]] ^= 0xFF
        prev, pending[0] = pending[0], (k, g.launch(slot))
        if prev is not None:
            collect(prev[0], prev[1].wait(copy=False))

    inflight = [issue(0)]
    for k in range(1, STEPS):
        inflight.append(issue(k))
        retire(*inflight.pop(0))
    retire(*inflight.pop(0))
    k, last = pending[0]
    collect(k, last.wait(copy=False))
    job.close()
    return out


def _fake_proof_step(step, i, a, b):
    # the gloo tests' ragged lengths: the longest proof changes from step to step, so does the width the all_reduce agrees on
    return (b"s%d-proof-%d-%d-%d|" % (step, i, a, b)) * (2 + (i * 7 + step * 5) % 9)


def async_gather(batch, device):
    """tests/test_distributed_cpu.py::_worker_async: scatter_descriptors (shape learnt from rank 0) and gather_proofs_async (width
    learnt by the all_reduce, staging slots created lazily per width) over five overlapping steps."""
    results, pending = [], None
    for step in range(5):
        inst = [(10 * step + i, 10 * step + i + 1) for i in range(7)]
        mine = batch.scatter_descriptors(inst, device)
        local = [(i, _fake_proof_step(step, i, a, b)) for i, a, b in mine]
        prev, pending = pending, batch.gather_proofs_async(local, 7, device)
        if prev is not None:
            results.append((prev.width, prev.wait()))
    results.append((pending.width, pending.wait()))
    return results


def pipelined_fake(batch, device):
    """tests/test_distributed_cpu.py::_worker_pipelined: a ProofGatherer without a width given up front, the sink called from
    threads in both forms, seven steps over the three slots, views on rank 0; an oversized proof is refused."""
    n_total, width, results, pending = 7, 64, [], [None]
    g = batch.ProofGatherer(n_total, device)

    def issue(step):
        mine = batch.scatter_descriptors([(10 * step + i, 10 * step + i + 1) for i in range(n_total)], device)
        put, slot = g.open(len(mine), width)

        def write(r, i, a, b):
            data = b"S%d:%d:%d:%d" % (step, i, a, b) * (1 + i % 3)
            if step % 2 == 0:
                put(r, i, data)
            else:
                address, cap = put.row_ptr(r)
                assert cap == width and len(data) <= cap
                ctypes.memmove(address, data, len(data))
                put.set(r, i, len(data))
        ths = [threading.Thread(target=write, args=(r, i, a, b)) for r, (i, a, b) in enumerate(mine)]
        [t.start() for t in ths]
        return ths, slot

    def retire(ths, slot):
        [t.join() for t in ths]
        prev, pending[0] = pending[0], g.launch(slot)
        if prev is not None:
            results.append([bytes(x) for x in prev.wait(copy=False)])

    inflight = [issue(0)]
    for step in range(1, 7):
        inflight.append(issue(step))
        retire(*inflight.pop(0))
    retire(*inflight.pop(0))
    results.append([bytes(x) for x in pending[0].wait(copy=False)])
    try:
        g.open(1, width)[0](0, 0, b"x" * (width + 1))
        overflow = "accepted"
    except ValueError:
        overflow = "refused"
    return results, overflow


def run_scatter(batch, device):
    """tests/test_distributed_cpu.py::_worker_run_scatter: five steps in one scatter read in any order (shape known), ragged steps with
    an empty and a short one (shape broadcast from rank 0), steps that are all empty, and a shape that does not hold the steps."""
    steps = [[(100 * k + i, 100 * k + i + 1) for i in range(7)] for k in range(5)]
    pend = batch.scatter_descriptor_steps(steps, device, shape=(5, 7))
    got = [(k, pend.step(k)) for k in (3, 0, 4, 1, 2, 3)]
    ragged = [[(1, 2), (3, 4), (5, 6)], [], [(9, 9)]]
    pend2 = batch.scatter_descriptor_steps(ragged, device)
    got2 = [pend2.step(k) for k in range(len(pend2))]
    pend3 = batch.scatter_descriptor_steps([[], []], device)
    got3 = [pend3.step(k) for k in range(len(pend3))]
    try:
        batch.scatter_descriptor_steps([[(0, 1)] * 4], device, shape=(1, 3))
        bad = None
    except ValueError as e:
        bad = str(e)
    return got, got2, got3, bad


def superseded(batch, device):
    """DescriptorScatter.run twice before the first result is read: every run lands in the same buffers."""
    s1 = [[(1, 2), (3, 4), (5, 6)], [(7, 8)]]
    s2 = [[(11, 12)], [(13, 14), (15, 16)]]
    sc = batch.DescriptorScatter(2, 3, device)

    def read(p, k):
        try:
            return ("ok", p.step(k))
        except RuntimeError as e:
            return ("error", str(e))
    p1 = sc.run(s1)
    p2 = sc.run(s2)
    late = read(p1, 0)  # run 1 read after run 2 was issued
    second = [read(p2, k) for k in range(2)]
    p3 = sc.run(s1)
    early = read(p3, 0)  # read before the next run: the result stays valid
    p4 = sc.run(s2)
    rest = read(p3, 1)
    fourth = [read(p4, k) for k in range(2)]
    return {"late": late, "second": second, "early": early, "rest": rest, "fourth": fourth}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["nccl", "gloo"], required=True)
    ap.add_argument("--device", choices=["cuda", "cpu"], required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--part", choices=["all", "pipelined"], default="all")
    ap.add_argument("--flip", default=None)
    args = ap.parse_args()
    flip = tuple(int(x) for x in args.flip.split(":")) if args.flip else None
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["RANK"], os.environ["WORLD_SIZE"] = "0", "1"
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    p3 = load_package()
    ok, msg = p3.is_available()
    if not ok:
        raise RuntimeError(msg)
    torch.cuda.set_device(0)
    from plonky3_mobile_amd import batch
    note = batch.init_process_group_for_batches(args.backend, 0)
    out = {"pg": note, "collective_stream": batch.collective_stream(args.device) is not None}
    out["pipelined"] = pipelined(p3, batch, args.device, flip)
    if args.part == "all":
        out["async"] = async_gather(batch, args.device)
        out["pipelined_fake"] = pipelined_fake(batch, args.device)
        out["run_scatter"] = run_scatter(batch, args.device)
        out["superseded"] = superseded(batch, args.device)
    dist.destroy_process_group()
    with open(args.out, "wb") as f:
        pickle.dump(out, f)


if __name__ == "__main__":
    main()
