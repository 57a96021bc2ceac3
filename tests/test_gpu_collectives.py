"""The bytes the multi-GPU batch path moves (plonky3_mobile_amd/batch.py), on the GPU branch: descriptor scatter and proof gather
over RCCL with device staging rows, pinned landings and per-slot events, checked against the oracle's proofs.

tests/test_distributed_cpu.py and tests/test_bench_cli.py cover the layout with gloo, CPU tensors and stub proofs; here the proofs
are real and every process group lives in a fresh child process (the pytest process has touched the GPU already): bench.py itself
for its real loop, tests/_collectives_child.py for the batch API.  Each child has its own port and time limit and runs once."""
import functools
import hashlib
import os
import pickle
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_collectives_child.py")
LOG_N, BATCH, THREADS, STEPS, WARMUP = 10, 7, 3, 5, 2
CONFIGS = {"poseidon2": ("poseidon2", False), "keccak-hiding": ("keccak", True)}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env(**extra):
    drop = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")
    env = {k: v for k, v in os.environ.items() if k not in drop and not k.startswith("P3HIP_BENCH_")}
    env.update(extra)
    return env


def _failed(what, rc, stderr):
    return "%s exited with %r\n--- stderr (tail) ---\n%s" % (what, rc, stderr[-6000:])


@functools.lru_cache(maxsize=None)
def _oracle_proof(a, config):
    from oracle import oracle as o
    hash, hiding = CONFIGS[config]
    kind = o.HASH_KECCAK if hash == "keccak" else o.HASH_POSEIDON2
    fp = o.FriParams(1, 0, 100, 16)
    if hiding:
        return o.prove_fib_air_hiding(a, a + 1, LOG_N, fp, hash=kind, seed=1)
    return o.prove_fib_air(a, a + 1, LOG_N, fp, hash=kind)


def _read_dump(d):
    """bench.py --dump-outputs: {slot: proof bytes}, {slot: length}, {slot: sha256 digest}."""
    import numpy as np

    def load(name):
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == np.float64, name
        return a
    slots = load("proof_slots").astype(int).tolist()
    lengths = dict(zip(slots, load("proof_lengths").astype(int).tolist()))
    digests = {s: np.asarray(h, dtype=">u4").tobytes() for s, h in zip(slots, load("proof_sha256").astype(np.uint32))}
    words = load("proof_words").astype(np.uint32)
    proofs = {s: words[r].astype("<u4").tobytes()[:lengths[s]] for r, s in enumerate(load("proof_words_slots").astype(int).tolist())}
    return proofs, lengths, digests


def _check_bench_proofs(p3, dump_dir, n_total, config):
    """The dump of the last timed step holds every instance of that step, each the oracle's proof, accepted by the verifier for its own
    statement and rejected for the neighbouring instance's public value."""
    proofs, lengths, digests = _read_dump(dump_dir)
    assert sorted(proofs) == list(range(n_total)) and sorted(lengths) == list(range(n_total))
    assert len(set(lengths.values())) == 1, lengths
    hash, hiding = CONFIGS[config]
    params = p3.FriParameters(1, 0, 100, 16)
    last = WARMUP + STEPS - 1
    bad = [i for i in range(n_total) if proofs[i] != _oracle_proof(last * n_total + i, config)]
    assert not bad, "gathered proofs that differ from the oracle's: instances %r" % bad
    for i in range(n_total):
        assert len(proofs[i]) == lengths[i] and hashlib.sha256(proofs[i]).digest() == digests[i], i
        a = last * n_total + i
        j = i + 1 if i + 1 < n_total else i - 1
        p3.verify_fib_air(proofs[i], a, a + 1, p3.fib_public_x(a, a + 1, 1 << LOG_N), LOG_N, params, hash=hash, hiding=hiding)
        an = last * n_total + j
        with pytest.raises(p3.P3HipError):
            p3.verify_fib_air(proofs[i], a, a + 1, p3.fib_public_x(an, an + 1, 1 << LOG_N), LOG_N, params, hash=hash, hiding=hiding)


def _bench_args(config, dump_dir):
    hash, hiding = CONFIGS[config]
    return ["--steps", str(STEPS), "--warmup", str(WARMUP), "--log-height", str(LOG_N), "--batch", str(BATCH),
            "--threads", str(THREADS), "--hash", hash, "--dump-outputs", dump_dir] + (["--hiding"] if hiding else [])


def _line(stdout):
    import json
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_bench_one_rank_rccl_gathers_the_oracles_proofs(p3, oracle, tmp_path, config):
    """bench.py with P3HIP_BENCH_FORCE_DIST=1 and the default backend: one rank, but RCCL scatters the descriptors and gathers the
    proofs through the device staging rows; 7 steps, so the last step's staging slot has been used twice before."""
    d = str(tmp_path / "dump")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + _bench_args(config, d),
                         env=_env(P3HIP_BENCH_FORCE_DIST="1", MASTER_PORT=str(_free_port())),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, _failed("bench.py (one rank, RCCL)", res.returncode, res.stderr)
    out = _line(res.stdout)
    assert "RCCL" in out["dist_backend"] and out["collectives"].startswith("rccl scatter/gather"), out["collectives"]
    _check_bench_proofs(p3, d, BATCH, config)


def _run_ranks(n, args, env_extra, timeout, tmp_path):
    """n bench.py ranks started here as a launcher would start them (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment):
    no process between this one and the ranks.  One deadline for all; a rank still running then is killed and the test fails."""
    import time
    port = _free_port()
    procs, logs = [], []
    for r in range(n):
        env = _env(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), **env_extra)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        so, se = open(tmp_path / ("rank%d.out" % r), "w+"), open(tmp_path / ("rank%d.err" % r), "w+")
        logs.append((so, se))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=so, stderr=se))
    deadline = time.monotonic() + timeout
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(timeout=max(1.0, deadline - time.monotonic())))
        except subprocess.TimeoutExpired:
            rcs.append("timeout")
    for p in procs:
        if p.poll() is None:
            p.kill()
            p.wait()
    texts = []
    for so, se in logs:
        so.seek(0)
        se.seek(0)
        texts.append((so.read(), se.read()))
        so.close()
        se.close()
    for r, rc in enumerate(rcs):
        assert rc == 0, _failed("bench.py rank %d of %d" % (r, n), rc, texts[r][1])
    return texts[0][0]


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_bench_two_ranks_gather_the_oracles_proofs(p3, oracle, tmp_path, backend):
    """Two bench.py ranks with real proofs: 14 instances a step, instance i -> rank i % 2, gathered on rank 0.  gloo: both ranks may
    share one GPU, the collectives move host tensors.  nccl: one GPU per rank, RCCL between them."""
    import torch
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("two-rank RCCL needs two GPUs; this node shows %d" % torch.cuda.device_count())
    d = str(tmp_path / "dump")
    args = _bench_args("poseidon2", d)
    if backend == "gloo":
        # through bench.py's own launcher, which touches no GPU itself on the gloo backend
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + args,
                             env=_env(P3HIP_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, _failed("bench.py --gpus 2 (gloo)", res.returncode, res.stderr)
        stdout = res.stdout
    else:
        stdout = _run_ranks(2, ["--gpus", "2"] + args, {}, 300, tmp_path)
    out = _line(stdout)
    assert out["world_size"] == 2 and [r["rank"] for r in out["ranks"]] == [0, 1]
    assert [r["proofs"] for r in out["ranks"]] == [BATCH * STEPS] * 2
    if backend == "nccl":
        assert "RCCL" in out["dist_backend"] and out["collectives"].startswith("rccl scatter/gather"), out["collectives"]
    else:
        assert out["dist_backend"] == "gloo" and out["collectives"].startswith("gloo scatter/gather"), out["collectives"]
    _check_bench_proofs(p3, d, 2 * BATCH, "poseidon2")


_CHILD_RUNS = {}


def _child(tmp_path_factory, backend, device, *extra):
    """One run of tests/_collectives_child.py per argument set in this session (the assertions on it are split over several tests)."""
    key = (backend, device) + extra
    if key not in _CHILD_RUNS:
        out = str(tmp_path_factory.mktemp("collectives") / "out.pkl")
        res = subprocess.run([sys.executable, CHILD, "--backend", backend, "--device", device, "--out", out] + list(extra),
                             env=_env(MASTER_PORT=str(_free_port())), capture_output=True, text=True, timeout=300)
        if res.returncode != 0:
            _CHILD_RUNS[key] = _failed("the collectives child (%s)" % " ".join(key), res.returncode, res.stderr)
        else:
            with open(out, "rb") as f:
                _CHILD_RUNS[key] = pickle.load(f)
    got = _CHILD_RUNS[key]
    assert not isinstance(got, str), got  # a failed child is not run again for the next test
    return got


BRANCHES = [("nccl", "cuda"), ("gloo", "cpu")]  # the device branch, and the host branch as the control


def _pipelined_mismatches(run):
    """(step, instance) of every gathered proof that differs from the oracle's, at collection and after the next step's collection."""
    at, after = set(), set()
    for k in range(7):
        exp = [_oracle_proof(k * 7 + i, "poseidon2") for i in range(7)]
        at |= {(k, i) for i in range(7) if run["proofs"][k][i] != exp[i]}
        if k < 6:
            after |= {(k, i) for i in range(7) if run["views_after_next"][k][i] != exp[i]}
    return at, after


@pytest.mark.parametrize("backend,device", BRANCHES)
def test_pipelined_loop_gathers_every_steps_proofs(p3, oracle, tmp_path_factory, backend, device):
    """bench.py's loop over the batch API with a real FibAirJob: every step's descriptors are the ones rank 0 sent, every step's
    gathered proofs (bytes sink and direct sink alternating) equal the oracle's, and wait(copy=False) views of step k still hold
    step k's bytes after step k + 1 was gathered and collected."""
    run = _child(tmp_path_factory, backend, device)
    assert run["collective_stream"] == (device == "cuda")
    pl = run["pipelined"]
    for k in range(7):
        assert pl["descriptors"][k] == [(i, 7 * k + i, 7 * k + i + 1) for i in range(7)], k
    assert sorted(pl["proofs"]) == list(range(7)) and sorted(pl["views_after_next"]) == list(range(6))
    assert pl["width"] == len(_oracle_proof(0, "poseidon2"))
    at, after = _pipelined_mismatches(pl)
    assert not at and not after, (sorted(at), sorted(after))


@pytest.mark.parametrize("backend,device", BRANCHES)
def test_fake_proof_workers_on_the_branch(p3, tmp_path_factory, backend, device):
    """The gloo tests' workers at world size 1 on this branch: ragged lengths with the width learnt by the all_reduce and slots made
    on first use, ProofGatherer with sinks from threads, one scatter for a whole run with and without the shape."""
    run = _child(tmp_path_factory, backend, device)
    from _collectives_child import _fake_proof_step
    assert len(run["async"]) == 5
    for step, (width, allp) in enumerate(run["async"]):
        exp = [_fake_proof_step(step, i, 10 * step + i, 10 * step + i + 1) for i in range(7)]
        assert allp == exp, step
        assert width == max(len(p) for p in exp), step
    results, overflow = run["pipelined_fake"]
    assert overflow == "refused" and len(results) == 7
    for step, allp in enumerate(results):
        assert allp == [b"S%d:%d:%d:%d" % (step, i, 10 * step + i, 10 * step + i + 1) * (1 + i % 3) for i in range(7)], step
    got, got2, got3, bad = run["run_scatter"]
    for k, shard in got:
        assert shard == [(i, 100 * k + i, 100 * k + i + 1) for i in range(7)], k
    assert got2 == [[(0, 1, 2), (1, 3, 4), (2, 5, 6)], [], [(0, 9, 9)]]
    assert got3 == [[], []]
    assert bad is not None and "announced" in bad


@pytest.mark.parametrize("backend,device", BRANCHES)
def test_superseded_descriptor_run_is_an_error(p3, tmp_path_factory, backend, device):
    """DescriptorScatter.run twice before the first result is read: both land in the same buffers, so the first result must not
    hand out the second run's descriptors.  It raises; a result read before the next run stays correct."""
    s = _child(tmp_path_factory, backend, device)["superseded"]
    run1 = [[(0, 1, 2), (1, 3, 4), (2, 5, 6)], [(0, 7, 8)]]
    run2 = [[(0, 11, 12)], [(0, 13, 14), (1, 15, 16)]]
    assert s["late"][0] == "error" and "superseded" in s["late"][1], s["late"]
    assert s["second"] == [("ok", run2[0]), ("ok", run2[1])]
    assert s["early"] == ("ok", run1[0]) and s["rest"] == ("ok", run1[1])
    assert s["fourth"] == [("ok", run2[0]), ("ok", run2[1])]


def test_negative_control_a_flipped_staging_byte_is_seen(p3, oracle, tmp_path_factory):
    """One byte of one proof inverted in its pinned staging row after the (direct) sink wrote it and before the gather: the comparison
    reports exactly that instance of that step, and every other proof of the run as equal."""
    pl = _child(tmp_path_factory, "nccl", "cuda", "--part", "pipelined", "--flip", "3:4:1000")["pipelined"]
    at, after = _pipelined_mismatches(pl)
    assert at == {(3, 4)} and after == {(3, 4)}, (sorted(at), sorted(after))
    good, flipped = _oracle_proof(3 * 7 + 4, "poseidon2"), pl["proofs"][3][4]
    assert len(flipped) == len(good) and [k for k in range(len(good)) if good[k] != flipped[k]] == [1000]
