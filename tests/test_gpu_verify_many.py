"""The batch verifier on the device (include/p3hip.h "batches of proofs verified ON THE DEVICE") against the host verifier, which is the
reference for reject codes, and the oracle's independently written verifier, which is the witness for accept.

The contract, with H the host verifier's code for the same bytes and public values (`_check_contract`):
  status == 0 exactly when H == 0;
  status == H when H is 10 / 11 / 13 / 14 / 15 and every field word of the proof is canonical;
  otherwise status is nonzero: H itself or VERIFY_MALFORMED (16)."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0x78000001
EQ_CODES = (10, 11, 13, 14, 15)
MIB = 1 << 20


def _kind(oracle, hash_name):
    return oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2


def _host_code(p3, proof, inst, log_n, fp, hash_name, hiding):
    lib = p3._lib.lib()
    buf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(proof if len(proof) else b"\0")
    fn = lib.p3hip_verify_fib_air_hiding if hiding else lib.p3hip_verify_fib_air_hash
    rc = fn(0 if hash_name == "poseidon2" else 1, buf, len(proof), inst[0], inst[1], inst[2], log_n, C.cast(fp._c(), C.c_void_p))
    p3.take_last_error()
    return rc


def _oracle_accepts(oracle, proof, inst, log_n, t, hash_name, hiding):
    fn = oracle.verify_fib_air_hiding if hiding else oracle.verify_fib_air
    return fn(proof, inst[0], inst[1], inst[2], log_n, oracle.FriParams(*t), hash=_kind(oracle, hash_name)) == 0


def _prove(p3, log_n, t, hash_name, hiding, insts, seed=5):
    """proofs of the PRODUCT's provers (a pool of two), with their instances (a, b, x)"""
    pool = p3.FibAirBatchProver(log_n, n_provers=2, params=p3.FriParameters(*t), hash=hash_name, hiding=hiding, seed=seed)
    try:
        proofs = pool.prove(insts)
    finally:
        pool.close()
    return proofs, [(a, b, p3.fib_public_x(a, b, 1 << log_n)) for a, b in insts]


def _monty(v):
    return ((v % P) << 32) % P


def _dev_batch(proofs, insts, stride):
    """the _dev entry's inputs as torch tensors: proofs at a stride, Montgomery public values, byte lengths"""
    import torch
    n = len(proofs)
    host = np.zeros((max(n, 1), stride), dtype=np.uint8)
    for i, p in enumerate(proofs):
        m = min(len(p), stride)
        host[i, :m] = np.frombuffer(p, dtype=np.uint8)[:m]
    pis = np.array([[_monty(v) for v in inst] for inst in insts], dtype=np.uint32).reshape(n, 3).view(np.int32)
    lens = np.array([len(p) for p in proofs], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(host).cuda(), torch.from_numpy(pis).cuda(), torch.from_numpy(lens).cuda()


def _verify_dev(ver, proofs, insts, with_lens=True, pad=0):
    d_proofs, d_pis, d_lens = _dev_batch(proofs, insts, ver.proof_len + pad)
    status, rejected = ver.verify_many_dev(d_proofs, d_pis, d_lens if with_lens else None, n=len(proofs))
    st = status.cpu().numpy().view(np.uint32)
    assert int(rejected.cpu()[0]) == int(np.count_nonzero(st)), "d_rejected is the count of nonzero codes"
    return st


def _check_contract(status, host, canonical, what):
    """-> the number of members under the code-equality clause"""
    under = 0
    for i, (s, h) in enumerate(zip(status, host)):
        s, h = int(s), int(h)
        assert (s == 0) == (h == 0), (what, i, s, h)
        if h in EQ_CODES and canonical[i]:
            assert s == h, (what, i, s, h)
            under += 1
        elif h != 0:
            assert s in (h, 16), (what, i, s, h)
    return under


def _t1(word):
    word = int(word)
    return (word + 1) % P if word < P else word ^ 1


def _tampered(proof, i, fn=_t1):
    w = np.frombuffer(proof, dtype=np.uint32).copy()
    w[i] = fn(w[i])
    return w.tobytes()


# ---- 1. accept ------------------------------------------------------------------------------------------------------------------
ACCEPT = [(log_n, (1, 0, 20, 8)) for log_n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)] + \
         [(9, t) for t in [(2, 0, 10, 4), (2, 2, 6, 5), (1, 3, 9, 0), (3, 1, 4, 10), (1, 8, 3, 2), (4, 0, 2, 1)]]


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
def test_accepts_what_the_provers_prove_and_rejects_a_neighbours_x(p3, oracle, hash_name, hiding):
    for log_n, t in ACCEPT:
        fp = p3.FriParameters(*t)
        proofs, insts = _prove(p3, log_n, t, hash_name, hiding, [(0, 1), (7, 11), (P - 1, 3), (123456789, 987654321 % P)])
        ver = p3.FibAirVerifier(log_n, fp, hash_name, hiding, max_proofs=4)
        try:
            assert all(len(p) == ver.proof_len for p in proofs)
            for st in (ver.verify_many(proofs, insts), _verify_dev(ver, proofs, insts), _verify_dev(ver, proofs, insts, with_lens=False, pad=12)):
                assert st.tolist() == [0, 0, 0, 0], (log_n, t, st)
            for p, inst in zip(proofs, insts):
                assert _oracle_accepts(oracle, p, inst, log_n, t, hash_name, hiding), (log_n, t)
            wrong = [(a, b, insts[(i + 1) % 4][2]) for i, (a, b, _) in enumerate(insts)]
            assert all(w[2] != i[2] for w, i in zip(wrong, insts))
            for st in (ver.verify_many(proofs, wrong), _verify_dev(ver, proofs, wrong)):
                assert st.tolist() == [10, 10, 10, 10], (log_n, t, st)
            assert _host_code(p3, proofs[0], wrong[0], log_n, fp, hash_name, hiding) == 10
        finally:
            ver.close()


# ---- 2. every word, tamper T1 -----------------------------------------------------------------------------------------------------
SMALL = (5, (1, 0, 5, 3))  # a proof of a few thousand words


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
def test_every_word_tampered_gives_the_host_verifiers_code(p3, hash_name, hiding):
    """Member i of ONE batch is the proof with word i changed ((w + 1) mod P for w < P, else w ^ 1: every field word stays canonical).
    At least 90 % of the members must fall under the code-equality clause: value and digest words far outnumber structural ones
    (the host verifier alone, on the oracle provers' proofs of these four configurations: 0.946 plain, 0.933 hiding)."""
    log_n, t = SMALL
    fp = p3.FriParameters(*t)
    proofs, insts = _prove(p3, log_n, t, hash_name, hiding, [(3, 4)])
    n = len(proofs[0]) // 4
    batch = [_tampered(proofs[0], i) for i in range(n)]
    ver = p3.FibAirVerifier(log_n, fp, hash_name, hiding, max_proofs=n)
    try:
        status = ver.verify_many(batch, insts * n)
        status_dev = _verify_dev(ver, batch, insts * n)
    finally:
        ver.close()
    host = [_host_code(p3, b, insts[0], log_n, fp, hash_name, hiding) for b in batch]
    assert np.array_equal(status, status_dev)
    under = _check_contract(status, host, [True] * n, (hash_name, hiding))
    print("%s hiding=%s: %d words, %d under the code-equality clause (%.3f)" % (hash_name, hiding, n, under, under / n))
    assert under >= 0.9 * n
    # 15 does not occur here (a changed final polynomial moves the proof of work or the five indices): the next test reaches it
    assert set(int(h) for h in host) >= {10, 11, 13, 14}


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
@pytest.mark.parametrize("log_n,t", [(1, (1, 0, 1, 0)), (2, (1, 0, 2, 0)), (2, (1, 1, 1, 0))])
def test_final_poly_mismatch_is_reported_as_15(p3, log_n, t, hash_name, hiding):
    """FinalPolyMismatch from ONE changed word: no proof-of-work bits and one or two queries over a tiny domain, so a changed
    final-polynomial word re-samples the same indices now and then; the openings then still hold and only the value at the end point
    differs.  Every final-polynomial word with 39 replacement values in one batch, member by member against the host verifier, which
    must answer 15 for some of them."""
    fp = p3.FriParameters(*t)
    proofs, insts = _prove(p3, log_n, t, hash_name, hiding, [(3, 4)])
    n_words, fpl = len(proofs[0]) // 4, 1 << t[1]
    batch = [_tampered(proofs[0], word, lambda w, k=k: (int(w) + k) % P)
             for word in range(n_words - 1 - 4 * fpl, n_words - 1) for k in range(1, 40)]
    host = [_host_code(p3, b, insts[0], log_n, fp, hash_name, hiding) for b in batch]
    assert 15 in host and set(host) <= {13, 14, 15}, sorted(set(host))
    ver = p3.FibAirVerifier(log_n, fp, hash_name, hiding, max_proofs=len(batch))
    try:
        for status in (ver.verify_many(batch, insts * len(batch)), _verify_dev(ver, batch, insts * len(batch))):
            assert _check_contract(status, host, [True] * len(batch), (log_n, t, hash_name, hiding)) == len(batch)
            assert status.tolist() == host
    finally:
        ver.close()


# ---- 3. malformed inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
def test_malformed_inputs(p3, hash_name, hiding):
    log_n, t = SMALL
    fp = p3.FriParameters(*t)
    proofs, insts = _prove(p3, log_n, t, hash_name, hiding, [(3, 4), (5, 6)])
    good, inst = proofs[0], insts[0]
    n_words = len(good) // 4
    rng = np.random.default_rng(20261017)
    # T2: the top bit of 300 sampled words, each member between two untouched neighbours
    batch, binst = [], []
    for i in rng.choice(n_words, size=300, replace=False):
        batch += [good, _tampered(good, int(i), lambda w: int(w) ^ 0x80000000), proofs[1]]
        binst += [inst, inst, insts[1]]
    # lengths off by 4 bytes either way, a version-swapped proof (the other wire format), an empty proof
    other, _ = _prove(p3, log_n, t, hash_name, not hiding, [(3, 4)])
    batch += [good[:-4], good, good + b"\0\0\0\0", proofs[1], other[0], good, b""]
    binst += [inst, inst, inst, insts[1], inst, inst, inst]
    host = [_host_code(p3, b, i, log_n, fp, hash_name, hiding) for b, i in zip(batch, binst)]
    ver = p3.FibAirVerifier(log_n, fp, hash_name, hiding, max_proofs=len(batch))
    small = p3.FibAirVerifier(log_n, fp, hash_name, hiding, max_proofs=7)
    try:
        for status in (ver.verify_many(batch, binst), _verify_dev(ver, batch, binst), small.verify_many(batch, binst)):  # `small` splits
            _check_contract(status, host, [False] * len(batch), (hash_name, hiding))
            good_at = [k for k, b in enumerate(batch) if b is good or b is proofs[1]]
            assert all(status[k] == 0 for k in good_at) and all(host[k] == 0 for k in good_at)
            assert all(status[k] != 0 for k in range(1, 900, 3)), "a flipped top bit is never accepted"
            assert status[-7] == 16 and status[-5] == 16 and status[-1] == 16 and status[-3] != 0
        # a version-swapped header in place (the same length): both reject
        swapped = _tampered(good, 1, lambda w: 3 - int(w))
        assert _host_code(p3, swapped, inst, log_n, fp, hash_name, hiding) == 1 and small.verify_many([swapped], [inst]).tolist() == [16]
        # n = 0, n = max_proofs, n > max_proofs
        assert small.verify_many([], []).tolist() == []
        assert small.verify_many([good] * 7, [inst] * 7).tolist() == [0] * 7
        assert _verify_dev(small, [good] * 7, [inst] * 7).tolist() == [0] * 7
        d_proofs, d_pis, d_lens = _dev_batch([good] * 8, [inst] * 8, small.proof_len)
        status, rejected = small.verify_many_dev(d_proofs, d_pis, d_lens, n=0)
        assert status.numel() == 0 and int(rejected.cpu()[0]) == 0
        with pytest.raises(p3.P3HipError, match="more proofs than the verifier was created for"):
            small.verify_many_dev(d_proofs, d_pis, d_lens, n=8)
        assert small.verify_many([good] * 8 + [swapped], [inst] * 9).tolist() == [0] * 8 + [16]  # split by the host entry
        # a public value that is no canonical word
        import torch
        d_pis2 = d_pis.clone()
        d_pis2[1, 2] = -1
        status, rejected = small.verify_many_dev(d_proofs, d_pis2, d_lens, n=3)
        assert status.cpu().tolist() == [0, 16, 0] and int(rejected.cpu()[0]) == 1
    finally:
        ver.close()
        small.close()
    with pytest.raises(p3.P3HipError, match="num_queries must be positive"):
        p3.FibAirVerifier(log_n, p3.FriParameters(1, 0, 0, 0), hash_name, hiding, max_proofs=1)
    with pytest.raises(p3.P3HipError, match="log_final_poly_len must be below"):
        p3.FibAirVerifier(3, p3.FriParameters(1, 5, 2, 0), hash_name, hiding, max_proofs=1)


# ---- 4. seeded random configurations ------------------------------------------------------------------------------------------------
def _cases(n, seed):
    """the space tests/test_gpu_random_configs.py draws from (a verifier needs at least one query, which that draw always has)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        hiding = bool(rng.integers(0, 2))
        log_n = int(rng.integers(1, 15))
        log_blowup = int(rng.integers(1, 4))
        top = log_n + 1 if hiding else log_n
        log_fpl = 0 if rng.integers(0, 3) == 0 else int(rng.integers(0, top))
        queries = int(rng.integers(1, 25))
        pow_bits = int(rng.integers(0, 13))
        hash_name = ("poseidon2", "keccak")[int(rng.integers(0, 2))]
        a, b = int(rng.integers(0, P)), int(rng.integers(0, P))
        gen_seed = int(rng.integers(0, 1 << 40))
        out.append((hiding, log_n, (log_blowup, log_fpl, queries, pow_bits), hash_name, a, b, gen_seed, int(rng.integers(0, 1 << 62))))
    return out


def test_random_configurations_follow_the_host_verifier(p3, oracle):
    for case in _cases(40, 20261017):
        hiding, log_n, t, hash_name, a, b, gen_seed, word_seed = case
        fp = p3.FriParameters(*t)
        pr = p3.FibAirProver(log_n, params=fp, hash=hash_name, hiding=hiding, seed=gen_seed)
        try:
            proof = pr.prove(a, b)
        finally:
            pr.close()
        inst = (a, b, p3.fib_public_x(a, b, 1 << log_n))
        assert p3.proof_len(log_n, fp, hash_name, hiding) == len(proof), case
        batch = [proof, proof, _tampered(proof, word_seed % (len(proof) // 4))]
        insts = [inst, (a, b, (inst[2] + 1) % P), inst]
        host = [_host_code(p3, p, i, log_n, fp, hash_name, hiding) for p, i in zip(batch, insts)]
        assert host[0] == 0 and host[1] == 10 and host[2] != 0, (case, host)
        assert _oracle_accepts(oracle, proof, inst, log_n, t, hash_name, hiding), case
        ver = p3.FibAirVerifier(log_n, fp, hash_name, hiding, max_proofs=3)
        try:
            for status in (ver.verify_many(batch, insts), _verify_dev(ver, batch, insts)):
                _check_contract(status, host, [True] * 3, case)
        finally:
            ver.close()


# ---- 5. at size -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_name,hiding", [("poseidon2", False), ("keccak", True)])
def test_eight_proofs_at_the_benchmarks_size(p3, hash_name, hiding):
    """cfg2: 2^20 rows, blowup 2, 100 queries, 16 proof-of-work bits.  One word in the LAST query's deepest FRI path (round 0) of one
    proof: that proof gives 14, as the host verifier does; the others stay accepted."""
    log_n, t = 20, (1, 0, 100, 16)
    fp = p3.FriParameters(*t)
    proofs, insts = _prove(p3, log_n, t, hash_name, hiding, [(k, k + 1) for k in range(8)], seed=1)
    log_big = log_n + 1 + (1 if hiding else 0)
    n_rounds = log_big - 1
    rounds = sum(4 + (5 if hiding else 0) + 1 + 8 * (log_big - 1 - r) for r in range(n_rounds))
    q_end = len(proofs[0]) // 4 - (1 + 4 + 1)  # behind the last query: the final polynomial (one element) and the witness
    word = q_end - rounds + 4 + (5 if hiding else 0) + 1 + 8 * 3 + 2  # round 0's path, fourth sibling, third word
    ver = p3.FibAirVerifier(log_n, fp, hash_name, hiding, max_proofs=8)
    try:
        assert ver.verify_many(proofs, insts).tolist() == [0] * 8
        assert _verify_dev(ver, proofs, insts).tolist() == [0] * 8
        bad = list(proofs)
        bad[5] = _tampered(proofs[5], word)
        assert ver.verify_many(bad, insts).tolist() == [0, 0, 0, 0, 0, 14, 0, 0]
        assert _verify_dev(ver, bad, insts).tolist() == [0, 0, 0, 0, 0, 14, 0, 0]
        assert _host_code(p3, bad[5], insts[5], log_n, fp, hash_name, hiding) == 14
    finally:
        ver.close()


# ---- 6. stream contract -----------------------------------------------------------------------------------------------------------
def test_two_verifiers_on_two_streams_and_a_verify_behind_an_upload(p3):
    import torch
    log_n, t = 8, (1, 0, 12, 4)
    fp = p3.FriParameters(*t)
    cfgs = [("poseidon2", False), ("keccak", True)]
    data = []
    for hash_name, hiding in cfgs:
        proofs, insts = _prove(p3, log_n, t, hash_name, hiding, [(k, 2 * k + 1) for k in range(6)])
        proofs[2] = _tampered(proofs[2], 30)  # an opened value
        host = [_host_code(p3, p, i, log_n, fp, hash_name, hiding) for p, i in zip(proofs, insts)]
        data.append((proofs, insts, host))
    vers = [p3.FibAirVerifier(log_n, fp, h, z, max_proofs=6) for h, z in cfgs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        ins = [_dev_batch(d[0], d[1], v.proof_len) for d, v in zip(data, vers)]
        torch.cuda.synchronize()
        outs = [[], []]
        for rep in range(4):  # interleaved on one host thread, nothing waited for in between
            for k in (0, 1):
                with torch.cuda.stream(streams[k]):
                    outs[k].append(vers[k].verify_many_dev(*ins[k], n=6))
        torch.cuda.synchronize()
        for k in (0, 1):
            for status, rejected in outs[k]:
                st = status.cpu().numpy().view(np.uint32)
                assert _check_contract(st, data[k][2], [True] * 6, cfgs[k]) == 1 and int(rejected.cpu()[0]) == 1
                assert [int(v) != 0 for v in st] == [False, False, True, False, False, False]
        # a prover's output copied to the device and verified behind the copy on the same stream, with no synchronise between
        prover = p3.FibAirProver(log_n, params=fp)
        try:
            with torch.cuda.stream(streams[0]):
                proof = prover.prove(9, 10)
                pinned = torch.frombuffer(bytearray(proof), dtype=torch.uint8).pin_memory()
                pis = torch.tensor([[_monty(9), _monty(10), _monty(p3.fib_public_x(9, 10, 1 << log_n))]], dtype=torch.int64).to(torch.int32).pin_memory()
                d_proof = pinned.to("cuda", non_blocking=True)
                d_pis = pis.to("cuda", non_blocking=True)
                status, rejected = vers[0].verify_many_dev(d_proof, d_pis, None, n=1, stride=vers[0].proof_len)
            streams[0].synchronize()
            assert status.cpu().tolist() == [0] and int(rejected.cpu()[0]) == 0
        finally:
            prover.close()
    finally:
        for v in vers:
            v.close()


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_create_verify_destroy_returns_device_memory(p3):
    """the method of tests/test_gpu_lifetime.py: free device memory after the cycles is where the warm-up cycles left it"""
    import torch
    log_n, t = 10, (1, 0, 8, 4)
    fp = p3.FriParameters(*t)
    proofs, insts = _prove(p3, log_n, t, "keccak", True, [(1, 2), (3, 4)])

    def cycle():
        for max_proofs in (2, 64):
            v = p3.FibAirVerifier(log_n, fp, "keccak", True, max_proofs=max_proofs)
            assert v.verify_many(proofs, insts).tolist() == [0, 0]
            assert _verify_dev(v, proofs, insts).tolist() == [0, 0]
            v.close()
        gc.collect()
        torch.cuda.empty_cache()

    for _ in range(3):
        cycle()
    base = _free_bytes()
    for _ in range(20):
        cycle()
    lost = base - _free_bytes()
    assert lost < 2 * MIB, "free device memory fell by %.1f MiB over 20 create / verify / destroy cycles" % (lost / MIB)
