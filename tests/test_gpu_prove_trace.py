"""GPU tests of proving a CALLER's FibonacciAir trace with caller public values (include/p3hip.h "a CALLER's trace"):
prove(&config, &FibonacciAir{}, trace, &pis) as the reference calls it (native/src/fib_air.rs:61,68-70).

A Fibonacci trace with its own public values gives the bytes of prove(a, b) (and of the oracle, which proves (a, b) only).
Any other trace is committed as given: its commitment is the oracle's commitment of the same matrix, and the proof, which
upstream's release builds also produce, is rejected by both verifiers.  check_fib_trace is compared with a numpy evaluation of
the same rules."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0x78000001
GFP = (1, 0, 10, 4)  # small FRI parameters: the one-launch hiding prover takes the small instances under them


def _params(p3, oracle, t=GFP):
    return p3.FriParameters(*t), oracle.FriParams(*t)


@functools.lru_cache(maxsize=None)
def _oracle_proof(log_n, hash_name, hiding, a, b, t=GFP):
    from oracle import oracle as o
    kind = o.HASH_KECCAK if hash_name == "keccak" else o.HASH_POSEIDON2
    if hiding:
        return o.prove_fib_air_hiding(a, b, log_n, o.FriParams(*t), hash=kind, seed=1)
    return o.prove_fib_air(a, b, log_n, o.FriParams(*t), hash=kind)


def _host(p3, t):
    return p3.host_u32(t)


def _to_dev(words):
    """numpy (n, 2) uint32 -> contiguous int32 device tensor with the same bits"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()


def _canon(oracle, w):
    return [int(v) for v in oracle.from_monty(np.asarray(w, dtype=np.uint32))]


def _fib(p3, oracle, a, b, n):
    """generate_trace_rows(a, b, n) on the host (any n); the device generator for the large powers of two"""
    if n >= 4096 and n & (n - 1) == 0:
        return np.ascontiguousarray(p3.host_u32(p3.generate_trace_rows(a, b, n)))
    return oracle.generate_trace_rows(a, b, n)


def _last_right(oracle, trace):
    return int(oracle.from_monty(np.asarray([trace[-1, 1]], dtype=np.uint32))[0])


def _assert_same(proof, ref, what):
    assert len(proof) == len(ref), (what, len(proof), len(ref))
    if proof != ref:
        w1, w2 = np.frombuffer(proof, np.uint32), np.frombuffer(ref, np.uint32)
        first = int(np.nonzero(w1 != w2)[0][0])
        pytest.fail("%s: proof words differ first at %d of %d" % (what, first, len(w1)))


# ---- 1. a Fibonacci trace with its own public values: the bytes of prove(a, b) and of the oracle ----
@pytest.mark.parametrize("log_n", [1, 3, 8, 12])
@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("profile", ["latency", "throughput"])
def test_fibonacci_trace_same_bytes(p3, oracle, log_n, hash_name, hiding, profile):
    a, b = 7, 11
    n = 1 << log_n
    gfp, _ = _params(p3, oracle)
    pr = p3.FibAirProver(log_n, params=gfp, hash=hash_name, hiding=hiding, profile=profile)
    try:
        pis = [a, b, p3.fib_public_x(a, b, n)]
        trace = p3.generate_trace_rows(a, b, n)
        dev = pr.prove_trace(trace, pis)
        host = pr.prove_trace(_host(p3, trace), pis)
        ref = pr.prove(a, b)
        _assert_same(dev, ref, "prove_trace_dev vs prove(a, b)")
        _assert_same(host, ref, "host entry vs prove(a, b)")
        _assert_same(ref, _oracle_proof(log_n, hash_name, hiding, a, b), "oracle")
    finally:
        pr.close()


def test_reference_instance_one_launch(p3, oracle):
    """The reference's own instance (fib_air.rs:28-72): n = 8, Keccak, hiding, create_test_fri_params(_, 2), seed 1 — the one-launch
    prover of the latency profile, now fed the caller's trace."""
    t = (2, 2, 2, 1)
    zfp, zofp = _params(p3, oracle, t)
    pr = p3.FibAirProver(3, params=zfp, hash="keccak", hiding=True, seed=1)
    try:
        trace = p3.generate_trace_rows(0, 1, 8)
        proof = pr.prove_trace(trace, [0, 1, 21])
        ref = oracle.prove_fib_air_hiding(0, 1, 3, zofp, hash=oracle.HASH_KECCAK, seed=1)
        _assert_same(proof, ref, "n = 8 Keccak hiding")
        _assert_same(pr.prove_trace(_host(p3, trace), [0, 1, 21]), ref, "host entry")
        assert oracle.verify_fib_air_hiding(proof, 0, 1, 21, 3, zofp, hash=oracle.HASH_KECCAK) == 0
    finally:
        pr.close()


@pytest.mark.parametrize("log_n,t", [(20, (1, 0, 20, 8)), (24, (2, 0, 20, 8))])
def test_large_fibonacci_trace_same_bytes_as_prove(p3, oracle, log_n, t):
    """2^20 (BASELINE cfg2's size) and the cfg3 shape (2^24 rows, blowup 4): prove_trace equals prove(a, b); no oracle."""
    gfp, _ = _params(p3, oracle, t)
    pr = p3.FibAirProver(log_n, params=gfp)
    try:
        n = 1 << log_n
        trace = p3.generate_trace_rows(3, 5, n)
        proof = pr.prove_trace(trace, [3, 5, _last_right(oracle, _host(p3, trace))])
        _assert_same(proof, pr.prove(3, 5), "2^%d" % log_n)
    finally:
        pr.close()


@pytest.mark.parametrize("hiding", [False, True])
def test_pool_prove_traces_equals_single_prover(p3, oracle, hiding):
    gfp, _ = _params(p3, oracle)
    log_n, n = 8, 256
    inst = [(i, 2 * i + 1) for i in range(16)]
    traces = [p3.generate_trace_rows(a, b, n) for a, b in inst]
    pis = [[a, b, p3.fib_public_x(a, b, n)] for a, b in inst]
    pool = p3.FibAirBatchProver(log_n, n_provers=4, params=gfp, hiding=hiding)
    try:
        proofs = pool.prove_traces(traces, pis)
    finally:
        pool.close()
    pr = p3.FibAirProver(log_n, params=gfp, hiding=hiding)
    try:
        for (a, b), pf in zip(inst, proofs):
            _assert_same(pf, pr.prove(a, b), "pool instance (%d, %d)" % (a, b))
    finally:
        pr.close()


def test_enqueue_trace_two_in_flight(p3, oracle):
    gfp, _ = _params(p3, oracle)
    log_n, n = 10, 1024
    pr = p3.FibAirProver(log_n, params=gfp)
    try:
        t1, t2 = p3.generate_trace_rows(1, 2, n), p3.generate_trace_rows(5, 8, n)
        p1, p2 = [1, 2, p3.fib_public_x(1, 2, n)], [5, 8, p3.fib_public_x(5, 8, n)]
        pr.enqueue_trace(t1, p1)
        pr.enqueue_trace(t2, p2)
        f1, f2 = pr.finish(), pr.finish()
        _assert_same(f1, pr.prove_trace(t1, p1), "first in flight")
        _assert_same(f2, pr.prove_trace(t2, p2), "second in flight")
        _assert_same(f1, pr.prove(1, 2), "first vs prove(a, b)")
    finally:
        pr.close()


# ---- 2 + 3. other traces: committed as given, proven, rejected ----
def _bad_cases(oracle, log_n):
    n = 1 << log_n
    rng = np.random.default_rng(1234 + log_n)
    rand = rng.integers(0, P, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    cases = [("random", rand, _canon(oracle, [rand[0, 0], rand[0, 1], rand[n - 1, 1]]))]
    fib = oracle.generate_trace_rows(7, 11, n)
    fib_pis = [7, 11, oracle.fib_public_x(7, 11, n)]
    for row in (0, n // 2 + 1, n - 1):
        bad = fib.copy()
        bad[row, 1] = np.uint32((int(bad[row, 1]) + 12345) % P)
        cases.append(("corrupt row %d" % row, bad, fib_pis))
    cases.append(("wrong x", fib, fib_pis[:2] + [(fib_pis[2] + 1) % P]))
    return cases


@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
def test_caller_trace_is_what_gets_committed(p3, oracle, hash_name):
    log_n = 8
    gfp, _ = _params(p3, oracle)
    kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
    pr = p3.FibAirProver(log_n, params=gfp, hash=hash_name)
    try:
        for what, trace, pis in _bad_cases(oracle, log_n):
            proof = pr.prove_trace(_to_dev(trace), pis)
            root, _ = oracle.mmcs_commit([oracle.coset_lde_batch(trace, gfp.log_blowup, p3.GENERATOR_MONTY, True)], kind)
            assert np.array_equal(np.frombuffer(proof[12:44], np.uint32), root), what
    finally:
        pr.close()


@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("log_n", [3, 8])
def test_bad_input_is_proven_and_rejected(p3, oracle, hash_name, hiding, log_n):
    gfp, ofp = _params(p3, oracle)
    kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
    pr = p3.FibAirProver(log_n, params=gfp, hash=hash_name, hiding=hiding)
    overify = oracle.verify_fib_air_hiding if hiding else oracle.verify_fib_air
    try:
        for what, trace, pis in _bad_cases(oracle, log_n):
            dev = _to_dev(trace)
            proof = pr.prove_trace(dev, pis)
            assert proof and pr.prove_trace(dev, pis) == proof, what  # produced and deterministic
            with pytest.raises(p3.P3HipError):
                p3.verify_fib_air(proof, *pis, log_n, params=gfp, hash=hash_name, hiding=hiding)
            assert overify(proof, *pis, log_n, ofp, hash=kind) != 0, what
    finally:
        pr.close()


@pytest.mark.parametrize("hiding", [False, True])
def test_no_state_leaks_between_paths(p3, oracle, hiding):
    gfp, _ = _params(p3, oracle)
    log_n = 9
    pr = p3.FibAirProver(log_n, params=gfp, hiding=hiding)
    try:
        first = pr.prove(4, 9)
        rand = np.random.default_rng(5).integers(0, P, size=(1 << log_n, 2), dtype=np.uint64).astype(np.uint32)
        pr.prove_trace(_to_dev(rand), [1, 2, 3])
        pr.prove_trace(rand, [4, 5, 6])  # host entry: the arena's trace slot
        assert pr.prove(4, 9) == first
    finally:
        pr.close()


# ---- 5. check_constraints ----
def _np_check(trace, pis_m):
    t = trace.astype(np.uint64)
    n = t.shape[0]
    l, r = t[:, 0], t[:, 1]
    m = np.where((l >= P) | (r >= P), 32, 0).astype(np.uint32)
    m[0] |= (1 if l[0] != pis_m[0] else 0) | (2 if r[0] != pis_m[1] else 0)
    if n > 1:
        m[:-1] |= np.where(l[1:] != r[:-1], 4, 0).astype(np.uint32)
        m[:-1] |= np.where(r[1:] != (l[:-1] + r[:-1]) % P, 8, 0).astype(np.uint32)
    m[n - 1] |= 16 if r[n - 1] != pis_m[2] else 0
    bad = np.nonzero(m)[0]
    if len(bad) == 0:
        return None, 0, 0
    return int(bad[0]), int(m[bad[0]]), int(len(bad))


def _checks(p3, oracle, trace, pis):
    pis_m = [int(v) for v in oracle.to_monty(np.array(pis, dtype=np.uint64))]
    got = p3.check_fib_trace(_to_dev(trace), pis)
    assert got == _np_check(trace, pis_m)
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 8, 129, 1 << 12, 1 << 22])
def test_check_fib_trace_agrees_with_numpy(p3, oracle, n):
    fib = _fib(p3, oracle, 2, 3, n)
    pis = [2, 3, _last_right(oracle, fib)]
    assert _checks(p3, oracle, fib, pis) == (None, 0, 0)
    # wrong public values: the boundary rules
    _checks(p3, oracle, fib, [3, 3, pis[2]])
    _checks(p3, oracle, fib, [2, 4, pis[2] + 1])
    # single corruptions at the boundaries and at the positions where the next row comes from another lane / tile / wave
    rows = sorted({0, 1, 62, 63, 64, 127, 128, 511, 512, n // 2, n - 2, n - 1} & set(range(n)))
    for row in rows:
        for col in (0, 1):
            bad = fib.copy()
            bad[row, col] = np.uint32((int(bad[row, col]) + 1) % P)
            _checks(p3, oracle, bad, pis)
    # a word >= P, and several corruptions at once
    bad = fib.copy()
    bad[n - 1, 0] = np.uint32(P + 5)
    _checks(p3, oracle, bad, pis)
    if n > 4:
        bad = fib.copy()
        for row in rows[1:]:
            bad[row, 0] = np.uint32(0xffffffff)
        got = _checks(p3, oracle, bad, pis)
        assert got[0] == rows[1] - 1 and got[2] >= len(rows) - 1


def test_check_fib_trace_unaligned_rows(p3, oracle):
    """A trace starting 8 bytes into its allocation (a row slice): the two-loads-per-lane form."""
    n = 1 << 12
    fib = oracle.generate_trace_rows(1, 1, n + 1)
    dev = _to_dev(fib)[1:]
    assert dev.data_ptr() % 16 == 8
    row1 = [int(v) for v in oracle.from_monty(fib[1])]
    pis = row1 + [oracle.fib_public_x(1, 1, n + 1)]
    pis_m = [int(v) for v in oracle.to_monty(np.array(pis, dtype=np.uint64))]
    assert p3.check_fib_trace(dev, pis) == _np_check(fib[1:], pis_m) == (None, 0, 0)
    bad = fib.copy()
    bad[300, 1] ^= 1
    assert p3.check_fib_trace(_to_dev(bad)[1:], pis) == _np_check(bad[1:], pis_m)


@pytest.mark.parametrize("hiding", [False, True])
def test_check_flag(p3, oracle, hiding):
    gfp, _ = _params(p3, oracle)
    log_n, n = 8, 256
    pr = p3.FibAirProver(log_n, params=gfp, hiding=hiding)
    try:
        fib = oracle.generate_trace_rows(7, 11, n)
        pis = [7, 11, oracle.fib_public_x(7, 11, n)]
        dev = _to_dev(fib)
        assert pr.prove_trace(dev, pis, check=True) == pr.prove_trace(dev, pis) == pr.prove(7, 11)
        bad = fib.copy()
        bad[77, 0] ^= 1
        with pytest.raises(p3.P3HipError) as e:
            pr.prove_trace(_to_dev(bad), pis, check=True)
        assert e.value.code == -1 and "constraints had nonzero value on row 76" in str(e.value)
        with pytest.raises(p3.P3HipError, match="row 255"):
            pr.prove_trace(fib, pis[:2] + [pis[2] + 1], check=True)  # host entry, wrong x
        assert pr.prove(7, 11) == pr.prove_trace(dev, pis)
    finally:
        pr.close()
    pool = p3.FibAirBatchProver(log_n, n_provers=2, params=gfp, hiding=hiding)
    try:
        with pytest.raises(p3.P3HipError, match="row 76"):
            pool.prove_traces([dev, _to_dev(bad)], [pis, pis], check=True)
    finally:
        pool.close()


# ---- 6. refusals, before anything is launched ----
def test_refusals(p3, oracle):
    import ctypes as C
    gfp, _ = _params(p3, oracle)
    log_n, n = 6, 64
    L = p3._lib.lib()
    pr = p3.FibAirProver(log_n, params=gfp)
    try:
        trace = p3.generate_trace_rows(7, 11, n)
        import torch
        torch.cuda.synchronize()
        good = pr.prove(7, 11)
        ok = (C.c_uint32 * 3)(*[int(v) for v in oracle.to_monty(np.array([7, 11, p3.fib_public_x(7, 11, n)], dtype=np.uint64))])
        tp = C.c_void_p(trace.data_ptr())
        out, ln = C.POINTER(C.c_uint8)(), C.c_size_t()
        BAD = -1
        # null pointers
        assert L.p3hip_fib_prover_prove_trace_dev(pr._h, None, ok, 0, C.byref(out), C.byref(ln)) == BAD
        assert L.p3hip_fib_prover_prove_trace_dev(pr._h, tp, None, 0, C.byref(out), C.byref(ln)) == BAD
        assert L.p3hip_fib_prover_prove_trace_dev(None, tp, ok, 0, C.byref(out), C.byref(ln)) == BAD
        assert L.p3hip_fib_prover_prove_trace_dev(pr._h, tp, ok, 0, None, C.byref(ln)) == BAD
        assert L.p3hip_fib_prover_enqueue_trace_dev(pr._h, None, ok) == BAD
        assert L.p3hip_fib_check_trace_dev(None, n, ok, C.byref(p3.fib_air.TraceCheck()), None) == BAD
        host = np.ascontiguousarray(p3.host_u32(trace))
        assert L.p3hip_fib_prover_prove_trace(pr._h, None, n, ok, 0, C.byref(out), C.byref(ln)) == BAD
        # host entry: n != 2^log_n
        for m in (n - 1, n // 2, 2 * n):
            assert L.p3hip_fib_prover_prove_trace(pr._h, C.c_void_p(host.ctypes.data), m, ok, 0, C.byref(out), C.byref(ln)) == BAD
        # a pis word >= P
        for k in range(3):
            badp = (C.c_uint32 * 3)(*ok)
            badp[k] = P
            assert L.p3hip_fib_prover_prove_trace_dev(pr._h, tp, badp, 0, C.byref(out), C.byref(ln)) == BAD
            assert L.p3hip_fib_prover_prove_trace(pr._h, C.c_void_p(host.ctypes.data), n, badp, 0, C.byref(out), C.byref(ln)) == BAD
        # unknown flag bits
        for flags in (2, 0x80000000, 3):
            assert L.p3hip_fib_prover_prove_trace_dev(pr._h, tp, ok, flags, C.byref(out), C.byref(ln)) == BAD
        assert "unknown flag" in (p3.take_last_error() or "")
        # the enqueue form belongs to the non-hiding prover
        assert pr.prove_trace(trace, [7, 11, p3.fib_public_x(7, 11, n)]) == good
    finally:
        pr.close()
    pool = p3.FibAirBatchProver(log_n, n_provers=2, params=gfp)
    try:
        badp = (C.c_uint32 * 6)(*ok, *ok)
        badp[4] = P
        ptrs = (C.c_void_p * 2)(trace.data_ptr(), trace.data_ptr())
        outs, lens = (C.POINTER(C.c_uint8) * 2)(), (C.c_size_t * 2)()
        assert L.p3hip_fib_batch_prove_traces_dev(pool._h, 2, ptrs, badp, 0, outs, lens) == BAD
        assert "instance 1" in (p3.take_last_error() or "")
        assert L.p3hip_fib_batch_prove_traces_dev(pool._h, 2, ptrs, ok, 4, outs, lens) == BAD
        nulls = (C.c_void_p * 2)(trace.data_ptr(), None)
        goodp = (C.c_uint32 * 6)(*ok, *ok)
        assert L.p3hip_fib_batch_prove_traces_dev(pool._h, 2, nulls, goodp, 0, outs, lens) == BAD
        assert pool.prove_traces([trace], [[7, 11, p3.fib_public_x(7, 11, n)]]) == [good]
    finally:
        pool.close()
    hp = p3.FibAirProver(3, params=gfp, hiding=True)
    try:
        t8 = p3.generate_trace_rows(0, 1, 8)
        with pytest.raises(p3.P3HipError, match="one proof at a time"):
            hp.enqueue_trace(t8, [0, 1, 21])
    finally:
        hp.close()
