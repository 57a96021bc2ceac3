"""GPU tests of the device TwoAdicFriPcs over caller matrices (plonky3-mobile_amd/pcs.py, csrc/pcs.hip.inc).

Byte pin: the fib_air instance driven THROUGH the PCS — commit the trace, replay the uni-stark prefix of the transcript, compute the
quotient here in numpy from get_evaluations_on_domain (oracle/stark.c:44-60), commit it with domain shift GENERATOR, open — gives,
with the header, roots and opened values put in front, the oracle prover's bytes and FibAirProver's bytes.
Generality: seeded random shapes; opened values against the evaluation of p3o_idft_batch coefficients, the library's verifier and
the Python verifier of pcs_ref.py accept, and both reject a perturbed word of every section."""
import gc

import numpy as np
import pytest

import pcs_ref as R
from pcs_ref import fib_quotient as _fib_quotient

pytestmark = pytest.mark.gpu
P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
# the eight FRI parameter sets of tests/test_gpu_prover.py
FRI_SETS = [(1, 0, 100, 16), (2, 0, 10, 4), (2, 2, 6, 5), (1, 3, 9, 0), (3, 1, 4, 10), (1, 0, 0, 0), (1, 8, 3, 2), (4, 0, 2, 1)]
FIRST_ROWS = [(0, 1), (7, 11), (P - 1, 1)]


def _fib_through_pcs(p3, pcs, hash, log_n, a, b):
    trace = p3.generate_trace_rows(a, b, 1 << log_n)  # a device tensor, committed where it lies
    pis = R.fib_pis(a, b, log_n)
    root_t, data_t = pcs.commit([(trace, None)])
    ch = p3.Challenger(hash)
    ch.observe([int(R.O.to_monty(log_n))] * 2)
    ch.observe_digest(root_t)
    ch.observe(pis)
    alpha = ch.sample_ext()
    low = p3.host_u32(pcs.get_evaluations_on_domain(data_t, 0, log_n))
    quot = _fib_quotient(low, log_n, pis, alpha)
    root_q, data_q = pcs.commit([(quot, p3.GENERATOR_MONTY)])
    ch.observe_digest(root_q)
    zeta = ch.sample_ext()
    zeta_next = R.ext_scale(zeta, R.two_adic_generator(log_n))
    opened, fri = pcs.open([(data_t, [[zeta, zeta_next]]), (data_q, [[zeta]])], ch)
    data_t.free()
    data_q.free()
    return R.fib_header(log_n, root_t, root_q, opened) + fri


def _same(proof, ref, what):
    assert len(proof) == len(ref), (what, len(proof), len(ref))
    if proof != ref:
        w1, w2 = np.frombuffer(proof, np.uint32), np.frombuffer(ref, np.uint32)
        pytest.fail("%s: proof words differ first at %d of %d" % (what, int(np.nonzero(w1 != w2)[0][0]), len(w1)))


@pytest.mark.parametrize("profile", ["latency", "throughput"])
@pytest.mark.parametrize("hash,kind", HASHES)
def test_fib_proof_through_the_pcs_equals_the_oracle_and_the_fib_prover(p3, oracle, hash, kind, profile):
    off = 3 * kind + (5 if profile == "throughput" else 0)
    cases = []
    for log_n in range(1, 15):  # every log_n with one applicable set and one first row, rotating
        valid = [t for t in FRI_SETS if t[1] < log_n]
        cases.append((log_n, valid[(log_n + off) % len(valid)], FIRST_ROWS[(log_n + off) % 3]))
    cases += [(9, t, FIRST_ROWS[(i + off) % 3]) for i, t in enumerate(FRI_SETS)]  # every set, where all eight apply
    assert {c[1] for c in cases} == set(FRI_SETS) and {c[2] for c in cases} == set(FIRST_ROWS)
    for log_n, t, (a, b) in cases:
        what = "%s %s log_n %d fri %s first row (%d, %d)" % (hash, profile, log_n, t, a, b)
        pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, profile)
        proof = _fib_through_pcs(p3, pcs, hash, log_n, a, b)
        pcs.free()
        _same(proof, oracle.prove_fib_air(a, b, log_n, oracle.FriParams(*t), hash=kind), what + " against the oracle")
        pr = p3.FibAirProver(log_n, params=p3.FriParameters(*t), hash=hash, profile=profile)
        _same(proof, pr.prove(a, b), what + " against FibAirProver")
        pr.close()


def _random_case(rng, log_h, widths_pool):
    n_rounds = int(rng.integers(1, 4))
    pool = [R.O.to_monty(rng.integers(0, P, 4, dtype=np.uint64)) for _ in range(int(rng.integers(1, 5)))]
    if rng.integers(0, 3) == 0:  # a base-field point off the LDE coset: z = 1 (the coset GENERATOR * <g> never holds 1)
        pool[0] = R.ext_from_base(R.ONE)
    rounds = []
    for _ in range(n_rounds):
        mats = []
        for _ in range(int(rng.integers(1, 5))):
            w = int(widths_pool[int(rng.integers(0, len(widths_pool)))])
            shift = int(R.O.to_monty(int(rng.integers(1, P)))) if rng.integers(0, 4) else None
            k = min(int(rng.integers(1, 4)), len(pool))
            pts = [pool[i] for i in rng.choice(len(pool), size=k, replace=False)]
            mats.append((R.O.to_monty(rng.integers(0, P, (1 << log_h, w), dtype=np.uint64)), shift, pts))
        rounds.append(mats)
    return rounds


def _check_case(p3, hash, kind, profile, t, log_h, rounds, horner_all=True):
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, profile)
    datas = [pcs.commit([(m, s) for m, s, _ in mats]) for mats in rounds]
    ch = p3.Challenger(hash)
    ch.observe(np.arange(1, 6, dtype=np.uint32))  # some transcript before the open
    before = ch.clone()
    opened, fri = pcs.open([(d, [pts for _, _, pts in mats]) for (_, d), mats in zip(datas, rounds)], ch)
    # opened values: evaluation of the interpolants' coefficients at z / s
    k = 0
    for mats in rounds:
        for m, s, pts in mats:
            for z in pts:
                w = m.shape[1]
                if horner_all:
                    assert np.array_equal(opened[k:k + w], R.opened_value(m, R.ONE if s is None else s, z)), (k, w)
                k += w
    assert k == len(opened)
    vr = [((root, [m.shape[1] for m, _, _ in mats]), [pts for _, _, pts in mats]) for (root, _), mats in zip(datas, rounds)]
    c = before.clone()
    p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, opened, fri, c)  # accepts
    assert np.array_equal(c.sample_ext(), ch.sample_ext())  # prover and verifier leave the same transcript
    ref = R.RefChallenger(kind)
    ref.observe(np.arange(1, 6, dtype=np.uint32))
    assert R.verify(kind, t, log_h, vr, opened, fri, ref) == 0
    for _, d in datas:
        d.free()
    pcs.free()
    return vr, before, opened, fri


def _rejected_by_both(p3, hash, kind, t, log_h, vr, before, opened, fri):
    try:
        p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, opened, fri, before.clone())
        lib = 0
    except p3.PcsRejected as e:
        lib = e.code
    ref = R.RefChallenger(kind)
    ref.observe(np.arange(1, 6, dtype=np.uint32))
    return lib != 0 and R.verify(kind, t, log_h, vr, opened, fri, ref) != 0


def _perturb_every_section(p3, rng, hash, kind, t, log_h, vr, before, opened, fri):
    bump = lambda v: (int(v) + 1) % P
    bad = opened.copy().reshape(-1)
    pos = int(rng.integers(0, bad.size))
    bad[pos] = bump(bad[pos])
    assert _rejected_by_both(p3, hash, kind, t, log_h, vr, before, bad.reshape(-1, 4), fri), ("opened", pos)
    words = np.frombuffer(fri, dtype=np.uint32)
    n_rounds, fpl = int(words[0]), 1 << t[1]
    q0, q1 = 2 + 8 * n_rounds, len(words) - 2 - 4 * fpl  # commit-phase roots | queries | final polynomial | witness
    sections = {"roots": (1, 1 + 8 * n_rounds), "queries": (q0, q1), "final polynomial": (q1 + 1, len(words) - 1), "witness": (len(words) - 1, len(words))}
    for name, (lo, hi) in sections.items():
        if hi <= lo:
            continue
        pos = int(rng.integers(lo, hi))
        b = words.copy()
        b[pos] = bump(b[pos])
        assert _rejected_by_both(p3, hash, kind, t, log_h, vr, before, opened, b.tobytes()), (name, pos)


@pytest.mark.parametrize("chunk", range(6))
def test_random_shapes_open_and_verify(p3, oracle, chunk):
    """64 seeded cases in 6 chunks: log_h 1..14 cycling, 1-3 rounds of 1-4 matrices, widths 1..48, 1-3 points per matrix from a pool
    of at most 4, random domain shifts, blowup 1..3, 1..24 queries, 0..12 proof-of-work bits; both hashes and profiles alternate."""
    for case in range(chunk, 64, 6):
        rng = np.random.default_rng(1000 + case)
        log_h = 1 + case % 14
        hash, kind = HASHES[(case // 2) % 2]
        profile = ("latency", "throughput")[case % 2]
        t = (int(rng.integers(1, 4)), int(rng.integers(0, min(log_h, 4))), int(rng.integers(1, 25)), int(rng.integers(0, 13)))
        rounds = _random_case(rng, log_h, np.arange(1, 49))
        vr, before, opened, fri = _check_case(p3, hash, kind, profile, t, log_h, rounds)
        _perturb_every_section(p3, rng, hash, kind, t, log_h, vr, before, opened, fri)


@pytest.mark.parametrize("hash,kind", HASHES)
def test_empty_first_proof_of_work_range_is_continued(p3, oracle, monkeypatch, hash, kind):
    """A first search range of 256 candidates against 12 proof-of-work bits: the host continues the search, the query phase is
    redone and the challenger fetched again; bytes and final transcript are the oracle's and the verifier's."""
    monkeypatch.setenv("P3HIP_GRIND_FIRST_LOG", "8")
    t, log_n, hit = (1, 0, 12, 12), 9, False
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
    for a in range(4):
        proof = _fib_through_pcs(p3, pcs, hash, log_n, a, a + 1)
        _same(proof, oracle.prove_fib_air(a, a + 1, log_n, oracle.FriParams(*t), hash=kind), "continued search, first row (%d, %d)" % (a, a + 1))
        hit |= int(oracle.from_monty(np.frombuffer(proof[-4:], np.uint32))[0]) >= 256
    assert hit, "no instance needed the continuation path: pick other instances"
    rng = np.random.default_rng(77)
    rounds = _random_case(rng, 6, np.arange(1, 20))
    _check_case(p3, hash, kind, "latency", t, 6, rounds)  # prover and verifier transcripts agree after a continued search too


@pytest.mark.parametrize("width,log_h", [(64, 9), (100, 7), (257, 6)])
def test_wide_matrices(p3, oracle, width, log_h):
    for i, (hash, kind) in enumerate(HASHES):
        rng = np.random.default_rng(width + i)
        t = (1 + i, 1, 5, 3)
        rounds = _random_case(rng, log_h, np.array([width, 3, width]))
        rounds[0][0] = (R.O.to_monty(rng.integers(0, P, (1 << log_h, width), dtype=np.uint64)),) + rounds[0][0][1:]
        vr, before, opened, fri = _check_case(p3, hash, kind, "latency", t, log_h, rounds)
        _perturb_every_section(p3, rng, hash, kind, t, log_h, vr, before, opened, fri)


def test_gates_that_need_a_device(p3, oracle):
    rng = np.random.default_rng(3)
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(1, 0, 2, 1))
    m8, m16 = (R.O.to_monty(rng.integers(0, P, (h, 3), dtype=np.uint64)) for h in (8, 16))
    z = R.O.to_monty(rng.integers(0, P, 4, dtype=np.uint64))
    with pytest.raises(p3.P3HipError, match="matrix 1 has height 16, matrix 0 has 8: mixed heights are not supported"):
        pcs.commit([(m8, None), (m16, None)])
    with pytest.raises(p3.P3HipError, match="zero matrices"):
        pcs.commit([])
    with pytest.raises(p3.P3HipError, match="9 matrices, a commitment holds at most 8"):
        pcs.commit([(m8, None)] * 9)
    with pytest.raises(p3.P3HipError, match="matrix 0: height must be a power of two"):
        pcs.commit([(m8[:6], None)])
    with pytest.raises(p3.P3HipError, match="matrix 0: domain shift must be a nonzero field element"):
        pcs.commit([(m8, 0)])
    (_, d8), (_, d16) = pcs.commit([(m8, None)]), pcs.commit([(m16, None)])
    ch = p3.Challenger()
    with pytest.raises(p3.P3HipError, match="round 1 matrix 0 has height 2\\^4, round 0 has 2\\^3: mixed heights are not supported"):
        pcs.open([(d8, [[z]]), (d16, [[z]])], ch)
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(4), 3)))
    with pytest.raises(p3.P3HipError, match="round 0 matrix 0 point 1 lies on the LDE coset"):
        pcs.open([(d8, [[z, on]])], ch)
    with pytest.raises(p3.P3HipError, match="5 rounds, an open takes at most 4"):
        pcs.open([(d8, [[z]])] * 5, ch)
    with pytest.raises(p3.P3HipError, match="more than 4 distinct opening points"):
        pcs.open([(d8, [[R.ext_from_base(int(R.O.to_monty(k))) for k in range(2, 5)]]), (d8, [[z, R.ext_from_base(R.ONE)]])], ch)
    with pytest.raises(p3.P3HipError, match="another hash configuration"):
        pcs.open([(d8, [[z]])], p3.Challenger("keccak"))
    with pytest.raises(p3.P3HipError, match="log_final_poly_len must be below"):
        p3.TwoAdicFriPcs(p3.FriParameters(1, 3, 2, 1)).open([(p3.TwoAdicFriPcs(p3.FriParameters(1, 3, 2, 1)).commit([(m8, None)])[1], [[z]])], ch)
    with pytest.raises(p3.P3HipError, match="log_blowup must be >= 1"):
        p3.TwoAdicFriPcs(p3.FriParameters(0, 0, 2, 1))
    # none of the refused calls moved the transcript; the object still works, and the view is a view of HBM
    assert np.array_equal(ch.sample_ext(), p3.Challenger().sample_ext())
    low = pcs.get_evaluations_on_domain(d8, 0, 3)
    assert low.is_cuda and tuple(low.shape) == (8, 3)
    lde = oracle.coset_lde_batch(m8, 1, p3.GENERATOR_MONTY, bit_reversed_out=True)
    assert np.array_equal(p3.host_u32(pcs.get_evaluations_on_domain(d8, 0, 4)), lde) and np.array_equal(p3.host_u32(low), lde[:8])
    opened, fri = pcs.open([(d8, [[z]])], p3.Challenger())
    assert np.array_equal(opened, R.opened_value(m8, R.ONE, z))


@pytest.mark.parametrize("hash,kind", HASHES)
def test_size_2_20(p3, oracle, hash, kind):
    """2^20 rows x {2, 4, 32} columns, blowup 2, 100 queries, 16 bits: verify accepts, one column's opened values are checked by
    evaluation of its coefficients, a second open on the same object gives the same bytes."""
    import torch
    log_h, t = 20, (1, 0, 100, 16)
    rng = np.random.default_rng(20 + kind)
    mats = [torch.randint(0, P, (1 << log_h, w), dtype=torch.int32, device="cuda") for w in (2, 4, 32)]
    shift = int(R.O.to_monty(12345))
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
    (r0, d0), (r1, d1) = pcs.commit([(mats[0], None)]), pcs.commit([(mats[1], shift), (mats[2], None)])
    z0, z1 = (R.O.to_monty(rng.integers(0, P, 4, dtype=np.uint64)) for _ in range(2))
    pts = [(d0, [[z0, z1]]), (d1, [[z0], [z1, z0]])]
    ch = p3.Challenger(hash)
    opened, fri = pcs.open(pts, ch)
    ch2 = p3.Challenger(hash)
    opened2, fri2 = pcs.open(pts, ch2)
    assert fri2 == fri and np.array_equal(opened, opened2) and np.array_equal(ch.sample_ext(), ch2.sample_ext())
    vr = [((r0, [2]), [[z0, z1]]), ((r1, [4, 32]), [[z0], [z1, z0]])]
    p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, opened, fri, p3.Challenger(hash))
    # column 5 of the 32-wide matrix at z1 (opened values 8 .. 39) and column 1 of the shifted one at z0 (4 .. 7)
    col = p3.host_u32(mats[2][:, 5:6].contiguous())
    assert np.array_equal(opened[8 + 5], R.opened_value(col, R.ONE, z1)[0])
    col = p3.host_u32(mats[1][:, 1:2].contiguous())
    assert np.array_equal(opened[4 + 1], R.opened_value(col, shift, z0)[0])
    bad = opened.copy()
    bad[20, 2] = (int(bad[20, 2]) + 1) % P
    with pytest.raises(p3.PcsRejected):
        p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, bad, fri, p3.Challenger(hash))


def test_device_memory_returns_after_create_commit_open_free_cycles(p3):
    import psutil
    import torch
    MIB = 1 << 20
    rng = np.random.default_rng(9)
    m = [p3.dev_u32(R.O.to_monty(rng.integers(0, P, (1 << 12, w), dtype=np.uint64))) for w in (3, 40)]
    z = R.O.to_monty(rng.integers(0, P, 4, dtype=np.uint64))

    def cycle(k):
        for hash in ("poseidon2", "keccak"):
            pcs = p3.TwoAdicFriPcs(p3.FriParameters(1, 1, 6, 4), hash, own_stream=bool(k & 1))
            _, d0 = pcs.commit([(m[0], None), (m[1], None)])
            _, d1 = pcs.commit([(m[1], p3.GENERATOR_MONTY)])
            pcs.open([(d0, [[z], [z]]), (d1, [[z]])], p3.Challenger(hash))
            pcs.open([(d1, [[z]])], p3.Challenger(hash))  # another shape: the arena is rebuilt
            d0.free()
            d1.free()
            pcs.free()
        gc.collect()
        torch.cuda.empty_cache()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    for k in range(3):
        cycle(k)
    me = psutil.Process()
    base, rss0 = free_bytes(), me.memory_info().rss
    for k in range(25):
        cycle(10 + k)
    lost, grown = base - free_bytes(), me.memory_info().rss - rss0
    # a leaked LDE (>= 0.1 MiB here), FRI arena or tree would cost >= 25 x that; a leaked pinned staging buffer shows in the RSS
    assert lost < 8 * MIB, "free device memory fell by %.1f MiB over 25 cycles" % (lost / MIB)
    assert grown < 64 * MIB, "resident host memory grew by %.1f MiB over 25 cycles" % (grown / MIB)
    print("device memory lost %.2f MiB, host RSS grown %.2f MiB over 25 cycles" % (lost / MIB, grown / MIB))
