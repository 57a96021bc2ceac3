"""GPU tests of the device HidingFriPcs over caller matrices (plonky3-mobile_amd/pcs.py HidingFriPcs, csrc/pcs_hiding.hip.inc), against
the reference prover of tests/pcs_hiding_ref.py (pinned to the oracle's bytes by tests/test_pcs_hiding_ref_host.py).

Byte pin: the hiding fib_air instance driven THROUGH the PCS (two hiding commits, a quotient commit computed here in numpy from
get_evaluations_on_domain, the randomization commit, one open) gives oracle.prove_fib_air_hiding's bytes.
Generality: seeded shapes; roots, stored LDEs, opened values, FriProof bytes and the next transcript sample equal the reference's.
Stream state, limits and lifetime as the plain PCS's tests have them."""
import gc

import numpy as np
import pytest

import pcs_hiding_ref as H
import pcs_ref as R

pytestmark = pytest.mark.gpu
P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
FRI_SETS = [(1, 0, 100, 16), (2, 0, 10, 4), (2, 2, 6, 5), (1, 3, 9, 0), (3, 1, 4, 10), (1, 0, 0, 0), (4, 0, 2, 1)]
FIRST_ROWS = [(0, 1), (7, 11), (P - 1, 1)]
PREFIX = np.arange(1, 6, dtype=np.uint32)


class _Com:
    def __init__(self, root, data):
        self.root, self.data = root, data


class _Dev:
    """the library's HidingFriPcs behind the five methods of pcs_hiding_ref.HidingPcs"""

    def __init__(self, p3, t, hash, profile="latency", nrc=4, mmcs_seed=1, pcs_seed=1):
        self.p3, self.nrc = p3, nrc
        self.pcs = p3.HidingFriPcs(p3.FriParameters(*t), hash, profile, nrc, mmcs_seed, pcs_seed)
        self.coms = []

    def _keep(self, rd):
        self.coms.append(_Com(*rd))
        return self.coms[-1]

    def commit(self, mats):
        return self._keep(self.pcs.commit(mats))

    def commit_quotient(self, chunks):
        return self._keep(self.pcs.commit_quotient(chunks))

    def commit_randomization(self, log_h):
        return self._keep(self.pcs.get_opt_randomization_poly_commitment(log_h))

    def open(self, rounds, ch):
        return self.pcs.open([(c.data, mp) for c, mp in rounds], ch)

    def rows(self, com, log_size, i=0):
        return self.p3.host_u32(self.pcs.get_evaluations_on_domain(com.data, i, log_size))

    def free(self):
        for c in self.coms:
            c.data.free()
        self.pcs.free()


def _same(proof, ref, what):
    assert len(proof) == len(ref), (what, len(proof), len(ref))
    if proof != ref:
        w1, w2 = np.frombuffer(proof, np.uint32), np.frombuffer(ref, np.uint32)
        pytest.fail("%s: words differ first at %d of %d" % (what, int(np.nonzero(w1 != w2)[0][0]), len(w1)))


@pytest.mark.parametrize("profile", ["latency", "throughput"])
@pytest.mark.parametrize("hash,kind", HASHES)
def test_hiding_fib_proof_through_the_pcs_equals_the_oracle(p3, oracle, hash, kind, profile):
    off = 3 * kind + (5 if profile == "throughput" else 0)
    for log_n in (1, 2, 3, 6, 10):
        valid = [t for t in FRI_SETS if t[1] < log_n + 1]
        for seed in (1, 7):
            t = valid[(log_n + off + seed) % len(valid)]
            a, b = FIRST_ROWS[(log_n + off + seed) % 3]
            what = "%s %s log_n %d fri %s seed %d first row (%d, %d)" % (hash, profile, log_n, t, seed, a, b)
            dev = _Dev(p3, t, hash, profile, 4, seed, seed)
            proof = H.fib_through(dev, p3.Challenger(hash), log_n, p3.generate_trace_rows(a, b, 1 << log_n), R.fib_pis(a, b, log_n), dev.rows)
            dev.free()
            _same(proof, oracle.prove_fib_air_hiding(a, b, log_n, oracle.FriParams(*t), hash=kind, seed=seed), what)
            if t[2]:
                assert oracle.verify_fib_air_hiding(proof, a, b, oracle.fib_public_x(a, b, 1 << log_n), log_n, oracle.FriParams(*t), hash=kind) == 0, what


# ---- general shapes ----
WIDTHS = (1, 2, 3, 16, 17, 59, 60, 61, 124, 125, 129, 448)
WQS = (1, 4, 5, 16, 65)
N_CASES = 24


_cases = {}


def _case(case):
    """the seeded shape `case` of 24, the reference prover's commitments with it, computed once; no device is touched"""
    if case not in _cases:
        _cases[case] = _make_case(case)
    return _cases[case]


def _make_case(case):
    rng = np.random.default_rng(8000 + case)
    log_h = 1 + case % 8
    hash, kind = HASHES[(case // 2) % 2]
    profile = ("latency", "throughput")[case % 2]
    nrc = (4, 1, 8)[case % 3]
    t = (1 + case % 3, int(rng.integers(0, min(log_h + 1, 4))), case % 9, int(rng.integers(0, 7)))
    # three widths a case, walking the list: with NRC = 4 the cases 0, 3, 6, ... take widths 0-2, 9-11, 6-8, 3-5, ...
    widths = [WIDTHS[(3 * case + i) % len(WIDTHS)] for i in range(3)]
    quotient = ((2, 4)[(case // 3) % 2], WQS[case % len(WQS)]) if case % 4 != 3 else None
    seeds = (int(rng.integers(1, 1 << 40)), int(rng.integers(1, 1 << 40)))
    ref = H.HidingPcs(kind, t, nrc, *seeds)
    plan, rounds = H.random_rounds(rng, ref, log_h, widths, quotient=quotient, randomization=case % 5 == 0, shifts=case % 2 == 0, max_cols=1500)
    return dict(log_h=log_h, hash=hash, kind=kind, profile=profile, nrc=nrc, t=t, seeds=seeds, ref=ref, plan=plan, rounds=rounds)


def _compare_commitments(dev, ref_rounds, dev_rounds, what):
    for r, ((rc, _), (dc, _)) in enumerate(zip(ref_rounds, dev_rounds)):
        assert np.array_equal(rc.root, dc.root), (what, "root of round", r)
        for i, lde in enumerate(rc.ldes):
            got = dev.rows(dc, len(lde).bit_length() - 1, i)
            assert got.shape == lde.shape and np.array_equal(got, lde), (what, "stored LDE of round %d matrix %d" % (r, i))


def _open_both(p3, c, dev, ref_rounds, dev_rounds, what):
    rch, dch = R.RefChallenger(c["kind"]), p3.Challenger(c["hash"])
    rch.observe(PREFIX)
    dch.observe(PREFIX)
    ro, rf = c["ref"].open(ref_rounds, rch)
    do, df = dev.open(dev_rounds, dch)
    assert do.shape == ro.shape and np.array_equal(do, ro), (what, "opened values")
    _same(df, rf, what + ": FriProof bytes")
    assert np.array_equal(dch.sample_ext(), rch.sample_ext()), (what, "transcript after the open")
    return do, df


@pytest.mark.parametrize("chunk", range(4))
def test_general_shapes_equal_the_reference_prover(p3, oracle, chunk):
    for case in range(chunk, N_CASES, 4):
        c = _case(case)
        what = "case %d (%s %s log_h %d nrc %d fri %s)" % (case, c["hash"], c["profile"], c["log_h"], c["nrc"], c["t"])
        dev = _Dev(p3, c["t"], c["hash"], c["profile"], c["nrc"], *c["seeds"])
        dr = H.run_plan(dev, c["plan"])
        _compare_commitments(dev, c["rounds"], dr, what)
        opened, fri = _open_both(p3, c, dev, c["rounds"], dr, what)
        if c["t"][2]:
            ch = p3.Challenger(c["hash"])
            ch.observe(PREFIX)
            dev.pcs.verify(H.verifier_rounds(c["rounds"]), c["log_h"], opened, fri, ch)
        dev.free()


def test_general_shapes_reach_what_they_are_meant_to(oracle):
    seen = set()
    for case in range(N_CASES):
        c = _case(case)
        seen |= {"log_h%d" % c["log_h"], "blowup%d" % c["t"][0], "nq%d" % c["t"][2], "nrc%d" % c["nrc"]}
        for what, arg, mpts in c["plan"]:
            if what == "commit":
                seen |= {"cw%d" % (m.shape[1] + c["nrc"]) for m, _ in arg} | {"w%d" % m.shape[1] for m, _ in arg}
                seen |= {"shift" if s is not None else "noshift" for _, s in arg}
            if what == "quotient":
                seen |= {"C%d" % len(arg), "wq%d" % arg[0].shape[1]}
            if what == "random":
                seen.add("random")
    want = ({"log_h%d" % k for k in range(1, 9)} | {"blowup1", "blowup2", "blowup3", "nq0", "nq8", "nrc1", "nrc4", "nrc8", "C2", "C4", "shift", "noshift",
            "random"} | {"cw%d" % w for w in (63, 64, 65, 128, 129)} | {"w%d" % w for w in WIDTHS} | {"wq%d" % w for w in WQS})
    assert want <= seen, sorted(want - seen)


def test_stored_lde_of_a_2_12_row_shape(p3, oracle):
    rng = np.random.default_rng(12)
    log_h, t = 12, (1, 2, 3, 2)
    plan = [("commit", [(R.rand_matrix(rng, log_h, 3), R.rand_shift(rng)), (R.rand_matrix(rng, log_h, 61), None)], [[R.rand_point(rng)], []]),
            ("quotient", [R.rand_matrix(rng, log_h, 5) for _ in range(4)], [[R.rand_point(rng)]] + [[]] * 3),
            ("random", log_h, [[]])]
    for hash, kind in HASHES:
        c = dict(kind=kind, hash=hash, ref=H.HidingPcs(kind, t, 4, 3, 5))
        dev = _Dev(p3, t, hash, "latency", 4, 3, 5)
        rr, dr = H.run_plan(c["ref"], plan), H.run_plan(dev, plan)
        _compare_commitments(dev, rr, dr, hash)
        _open_both(p3, c, dev, rr, dr, hash)
        dev.free()


@pytest.mark.parametrize("hash,kind", HASHES)
def test_streams_advance_across_calls_and_refused_calls_draw_nothing(p3, oracle, hash, kind):
    rng = np.random.default_rng(50 + kind)
    log_h, t = 3, (1, 1, 4, 2)
    A = [(R.rand_matrix(rng, log_h, 2), None), (R.rand_matrix(rng, log_h, 17), R.rand_shift(rng))]
    B = [(R.rand_matrix(rng, log_h, 5), None)]
    z0, z1 = R.rand_point(rng), R.rand_point(rng)
    ref, dev = H.HidingPcs(kind, t, 4, 11, 13), _Dev(p3, t, hash, "latency", 4, 11, 13)
    c = dict(kind=kind, hash=hash, ref=ref)
    ra, da = ref.commit(A), dev.commit(A)
    # refused calls, each between two calls whose bytes are compared with the reference's: none of them draws
    m8, m16 = R.rand_matrix(rng, 3, 3), R.rand_matrix(rng, 4, 3)
    with pytest.raises(p3.P3HipError, match="matrix 1 has height 16, matrix 0 has 8: mixed heights are not supported"):
        dev.pcs.commit([(m8, None), (m16, None)])
    with pytest.raises(p3.P3HipError, match="5 matrices, a hiding commitment holds at most 4"):
        dev.pcs.commit([(m8, None)] * 5)
    with pytest.raises(p3.P3HipError, match="3 chunks: the blinding needs a power of two"):
        dev.pcs.commit_quotient([m8] * 3)
    with pytest.raises(p3.P3HipError, match="1 chunks: the blinding needs a power of two"):
        dev.pcs.commit_quotient([m8])
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_h + 2), 3)))
    ch = p3.Challenger(hash)
    with pytest.raises(p3.P3HipError, match="round 0 matrix 1 point 0 lies on the LDE coset"):
        dev.pcs.open([(da.data, [[z0], [on]])], ch)
    plain = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
    _, dp = plain.commit([(m8, None)])
    with pytest.raises(p3.P3HipError, match="round 1 holds plain prover data, this PCS is hiding"):
        dev.pcs.open([(da.data, [[z0], [z0]]), (dp, [[z0]])], ch)
    with pytest.raises(p3.P3HipError, match="round 0 holds hiding prover data, this PCS is not hiding"):
        plain.open([(da.data, [[z0], [z0]])], ch)
    with pytest.raises(p3.P3HipError, match="this PCS is not hiding"):
        p3.HidingFriPcs.commit_quotient(plain, [m8, m8])
    assert np.array_equal(ch.sample_ext(), p3.Challenger(hash).sample_ext())  # no refused open moved the transcript
    dp.free()
    plain.free()
    _compare_commitments(dev, [(ra, None)], [(da, None)], "first commit")
    _open_both(p3, c, dev, [(ra, [[z0, z1], [z0]])], [(da, [[z0, z1], [z0]])], "first open")
    rb, db = ref.commit(B), dev.commit(B)
    rq, dq = ref.commit_quotient([m8, m8 + 0]), dev.commit_quotient([m8, m8 + 0])
    _compare_commitments(dev, [(rb, None), (rq, None)], [(db, None), (dq, None)], "second commits")
    pts = [[z1], [z1, z0]]
    _open_both(p3, c, dev, [(rb, [[z1]]), (ra, pts), (rq, [[z0], []])], [(db, [[z1]]), (da, pts), (dq, [[z0], []])], "second open")
    _open_both(p3, c, dev, [(rb, [[z1]])], [(db, [[z1]])], "third open, another shape")
    dev.free()


@pytest.mark.parametrize("hash,kind", HASHES)
def test_fills_in_several_pieces_give_the_same_streams(p3, oracle, monkeypatch, hash, kind):
    """pieces of 2^10 elements instead of 2^26: every fill of this shape (draws of 2^7 x 25 and x 13, 2^9 x 4 salts per matrix and both at
    once, the t draws, the randomization matrix, the FRI salts) is split, the streams continue from piece to piece"""
    monkeypatch.setenv("P3HIP_PCS_FILL_PIECE_LOG", "10")
    rng = np.random.default_rng(60 + kind)
    log_h, t = 7, (1, 1, 5, 2)
    plan = [("commit", [(R.rand_matrix(rng, log_h, 17), None), (R.rand_matrix(rng, log_h, 5), R.rand_shift(rng))], [[R.rand_point(rng)], []]),
            ("quotient", [R.rand_matrix(rng, log_h, 5) for _ in range(4)], [[R.rand_point(rng)]] + [[]] * 3),
            ("random", log_h, [[R.rand_point(rng)]])]
    c = dict(kind=kind, hash=hash, ref=H.HidingPcs(kind, t, 4, 21, 22))
    dev = _Dev(p3, t, hash, "latency", 4, 21, 22)
    rr, dr = H.run_plan(c["ref"], plan), H.run_plan(dev, plan)
    _compare_commitments(dev, rr, dr, hash)
    _open_both(p3, c, dev, rr, dr, hash)
    dev.free()


def test_limits(p3, oracle):
    import torch
    rng = np.random.default_rng(24)
    z = [R.rand_point(rng) for _ in range(4)]
    # a domain of exactly 2^24 points is accepted, 2^25 refused
    pcs = p3.HidingFriPcs(p3.FriParameters(1, 0, 0, 0), "poseidon2", "latency", 1, 1, 1)
    m = torch.randint(0, P, (1 << 23, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(p3.P3HipError, match=r"LDE domain above 2\^24 points"):
        pcs.commit([(m, None)])
    with pytest.raises(p3.P3HipError, match=r"LDE domain above 2\^24 points"):
        pcs.get_opt_randomization_poly_commitment(23)
    root, d = pcs.commit([(m[:1 << 22], None)])
    assert d.dims == [(1 << 23, 2)]
    ch = p3.Challenger()
    opened, fri = pcs.open([(d, [[z[0]]])], ch)
    assert opened.shape == (2, 4) and len(fri) == 4 * (1 + 8 * 23 + 1 + 1 + 4 + 1)
    # a second object with the same seeds commits the same matrix to the same root
    d.free()
    pcs.free()
    pcs = p3.HidingFriPcs(p3.FriParameters(1, 0, 0, 0), "poseidon2", "latency", 1, 1, 1)
    root2, d = pcs.commit([(m[:1 << 22], None)])
    assert np.array_equal(root, root2)
    d.free()
    pcs.free()
    del m
    # the 8192nd batched column is accepted, the 8193rd refused with the transcript untouched; h = 2
    t = (1, 0, 3, 1)
    wide, one = R.rand_matrix(rng, 1, 2044), R.rand_matrix(rng, 1, 1)
    ref, dev = H.HidingPcs(0, t, 4, 2, 3), _Dev(p3, t, "poseidon2", "latency", 4, 2, 3)
    with pytest.raises(p3.P3HipError, match=r"matrix 0: width must be in \[1, 8188\]"):
        dev.pcs.commit([(R.rand_matrix(rng, 1, 8189), None)])
    rr, dr = ref.commit([(wide, None), (one, None)]), dev.commit([(wide, None), (one, None)])
    ch = p3.Challenger()
    ch.observe(PREFIX)
    with pytest.raises(p3.P3HipError, match="round 0 matrix 1 point 0: more than 8192 batched columns"):
        dev.pcs.open([(dr.data, [z, [z[0]]])], ch)
    fresh = p3.Challenger()
    fresh.observe(PREFIX)
    assert np.array_equal(ch.sample_ext(), fresh.sample_ext())
    opened, _ = _open_both(p3, dict(kind=0, hash="poseidon2", ref=ref), dev, [(rr, [z, []])], [(dr, [z, []])], "8192 columns")
    assert len(opened) == 8192
    dev.free()


def test_device_memory_returns_after_create_commit_open_free_cycles(p3):
    import psutil
    import torch
    MIB = 1 << 20
    rng = np.random.default_rng(9)
    m = [p3.dev_u32(R.rand_matrix(rng, 12, w)) for w in (3, 40)]
    q = [p3.dev_u32(R.rand_matrix(rng, 12, 4)) for _ in range(4)]
    z = R.rand_point(rng)

    def cycle(k):
        hash = ("poseidon2", "keccak")[k & 1]
        pcs = p3.HidingFriPcs(p3.FriParameters(1, 1, 6, 4), hash, own_stream=bool(k & 2))
        if k & 1:  # two shapes alternate
            _, d0 = pcs.commit([(m[0], None), (m[1], None)])
            _, d1 = pcs.commit_quotient(q)
            pcs.open([(d0, [[z], [z]]), (d1, [[z]] * 4)], p3.Challenger(hash))
        else:
            _, d0 = pcs.commit([(m[1], p3.GENERATOR_MONTY)])
            _, d1 = pcs.get_opt_randomization_poly_commitment(12)
            pcs.open([(d1, [[z]]), (d0, [[z]])], p3.Challenger(hash))
            pcs.open([(d0, [[z]])], p3.Challenger(hash))  # another shape: the arena is rebuilt
        d0.free()
        d1.free()
        pcs.free()
        gc.collect()
        torch.cuda.empty_cache()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    for k in range(4):
        cycle(k)
    me = psutil.Process()
    base, rss0 = free_bytes(), me.memory_info().rss
    for k in range(25):
        cycle(10 + k)
    lost, grown = base - free_bytes(), me.memory_info().rss - rss0
    # tests/test_gpu_lifetime.py's tolerance: a leaked LDE, salt matrix, scratch buffer or FRI arena would cost >= 25 x 0.1 MiB and more
    assert lost < 8 * MIB, "free device memory fell by %.1f MiB over 25 cycles" % (lost / MIB)
    assert grown < 64 * MIB, "resident host memory grew by %.1f MiB over 25 cycles" % (grown / MIB)
    print("device memory lost %.2f MiB, host RSS grown %.2f MiB over 25 cycles" % (lost / MIB, grown / MIB))
