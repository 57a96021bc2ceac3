"""GPU tests of the device TwoAdicFriPcs against the reference prover of tests/pcs_ref.py (open: oracle/stark.c:71-154 restated for
any shape, pinned to the oracle's fib_air bytes in tests/test_pcs_ref_host.py), on the shapes, values and object states that
tests/test_gpu_pcs.py does not enter.  Where the reference prover is affordable (LDE <= 2^11 rows, <= 600 batched columns, and the
one 8192-column shape of 16 rows) a case asserts equal opened values, equal FriProof bytes and an equal next sample of the two
challengers; the larger shapes and the closed forms say in their docstrings what they assert instead.  Every test names the kernel
branch, instantiation or host line of csrc/pcs.hip.inc it aims at."""
import numpy as np
import pytest

import pcs_ref as R
import structured_inputs as S

pytestmark = pytest.mark.gpu
P = R.P
HASHES = [("poseidon2", 0), ("keccak", 1)]
PROFILES = ("latency", "throughput")
PREFIX = np.arange(1, 6, dtype=np.uint32)  # some transcript before the open


def _same(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    if got != ref:
        w1, w2 = np.frombuffer(got, np.uint32), np.frombuffer(ref, np.uint32)
        pytest.fail("%s: FriProof words differ first at %d of %d" % (what, int(np.nonzero(w1 != w2)[0][0]), len(w1)))


def _commit_all(pcs, rounds):
    return [pcs.commit([(m, s) for m, s, _ in mats]) for mats in rounds]


def _open(pcs, datas, rounds, ch):
    return pcs.open([(d, [pts for _, _, pts in mats]) for (_, d), mats in zip(datas, rounds)], ch)


_refs = {}


def _reference(key, kind, t, log_h, rounds, prefix=PREFIX, prepare=None):
    """the reference prover's (opened, bytes, roots, next sample) of one case, computed once per key"""
    if key is None or key not in _refs:
        ch = R.RefChallenger(kind)
        if prepare is not None:
            prepare(ch)
        else:
            ch.observe(prefix)
        opened, fri, roots = R.open_with_roots(kind, t, log_h, rounds, ch)
        out = (opened, fri, roots, ch.sample_ext())
        if key is None:
            return out
        _refs[key] = out
    return _refs[key]


def _equals_reference(what, got, ref):
    (opened, fri, roots, nxt), (ropened, rfri, rroots, rnxt) = got, ref
    for r, (a, b) in enumerate(zip(roots, rroots)):
        assert np.array_equal(a, b), (what, "root of round", r)
    assert opened.shape == ropened.shape, (what, opened.shape, ropened.shape)
    if not np.array_equal(opened, ropened):
        pytest.fail("%s: opened values differ first at value %d of %d" % (what, int(np.nonzero((opened != ropened).any(axis=1))[0][0]), len(opened)))
    _same(fri, rfri, what)
    assert np.array_equal(nxt, rnxt), (what, "the transcripts part after the open")


def _device(p3, hash, profile, t, rounds, prepare=None, pcs=None, own_stream=False):
    """commit and open on a device PCS -> (opened, bytes, roots, next sample of the caller's challenger)"""
    mine = pcs is None
    if mine:
        pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, profile, own_stream=own_stream)
    datas = _commit_all(pcs, rounds)
    ch = p3.Challenger(hash)
    if prepare is not None:
        prepare(ch)
    else:
        ch.observe(PREFIX)
    opened, fri = _open(pcs, datas, rounds, ch)
    for _, d in datas:
        d.free()
    if mine:
        pcs.free()
    return opened, fri, [r for r, _ in datas], ch.sample_ext()


def _pin(p3, what, hash, kind, profile, t, log_h, rounds, key=None, **kw):
    got = _device(p3, hash, profile, t, rounds, **kw)
    _equals_reference(what, got, _reference(key, kind, t, log_h, rounds, prepare=kw.get("prepare")))
    return got


# ---------------------------------------------------------------- bytes on general shapes
@pytest.mark.parametrize("chunk", range(12))
def test_seeded_shapes_give_the_reference_bytes(p3, oracle, chunk):
    """48 seeded cases of pcs_ref.random_case in 12 chunks: log_h 1..8 cycling, blowup 1..3 (LDE <= 2^11 rows), 0..24 queries,
    0..8 proof-of-work bits, both hashes and profiles alternating.  Guards the whole of Pcs::open on general shapes: the order of
    the sections with several rounds and matrices (put_fri, query_gather_kernel over core.trees), the first proof-of-work witness
    (the smallest), num_queries = 0 (no query_gather launch), matrices without points (`if (!mt.np) continue`), repeated points
    (the zs[] de-duplication) and pcs_bary_kernel<1..4>."""
    for case in range(chunk, 48, 12):
        rng = np.random.default_rng(5000 + case)
        log_h = 1 + case % 8
        hash, kind = HASHES[(case // 2) % 2]
        t = (int(rng.integers(1, 4)), int(rng.integers(0, min(log_h, 4))), int(rng.integers(0, 25)) if case % 6 else 0, int(rng.integers(0, 9)))
        rounds = R.random_case(rng, log_h)
        _pin(p3, "case %d %s log_h %d fri %s" % (case, hash, log_h, t), hash, kind, PROFILES[case % 2], t, log_h, rounds)


# ---------------------------------------------------------------- named shapes
@pytest.mark.parametrize("w", [1, 16, 17, 64, 65])
def test_four_points_on_one_matrix(p3, oracle, w):
    """pcs_bary_kernel<4>, pcs_inv_denoms_kernel<4> and np = 4 in pcs_reduced_tail, on both sides of the narrow / tile threshold
    (w <= 16) and of the 64-column tile.  Taking pidx[3] for pidx[0] in the barycentric kernel changes the fourth point's values."""
    for i, (hash, kind) in enumerate(HASHES):
        rng = np.random.default_rng(100 * w + i)
        _pin(p3, "%s width %d" % (hash, w), hash, kind, PROFILES[i], (1 + i, 1, 5, 3), 5, R.four_point_case(rng, 5, w))


@pytest.mark.parametrize("hash,kind", HASHES)
def test_matrices_and_a_round_without_points(p3, oracle, hash, kind):
    """`if (!mt.np) continue` in both launch loops of Pcs::open and the `first` flag: matrix 0 has no point, so the first matrix
    that stores ro instead of adding to it is matrix 1; dropping the flag's hand-over adds stale arena words into ro."""
    rng = np.random.default_rng(43 + kind)
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(2 - kind, 1, 4, 2), hash)
    for i in range(2):  # twice on one object with other data: the second open finds the first one's ro in the kept arena
        rounds = R.empty_point_case(rng, 4)
        _pin(p3, "%s open %d" % (hash, i), hash, kind, "latency", (2 - kind, 1, 4, 2), 4, rounds, pcs=pcs)
    pcs.free()


@pytest.mark.parametrize("hash,kind", HASHES)
def test_the_same_point_twice_in_one_list(p3, oracle, hash, kind):
    """the de-duplication of points in Pcs::open (one d / xd row per distinct point, two pairs that share it)"""
    rng = np.random.default_rng(45 + kind)
    _pin(p3, hash, hash, kind, "latency", (1, 0, 5, 1), 3, R.repeated_point_case(rng, 3))


@pytest.mark.parametrize("log_h,log_blowup", [(1, 1), (3, 2)])
def test_lde_below_64_rows(p3, oracle, log_h, log_blowup):
    """pcs_reduced_tile_kernel with rows < 64 (the zero-filled rows of the tile and `lane < rows` before the tail) and the
    barycentric kernel with fewer rows than one wave step, at widths 17, 64, 65; LDEs of 4 and 32 rows."""
    for i, w in enumerate((17, 64, 65)):
        hash, kind = HASHES[i % 2]
        rng = np.random.default_rng(10 * w + log_h)
        z = [R.rand_point(rng) for _ in range(2)]
        rounds = [[(R.rand_matrix(rng, log_h, w), R.rand_shift(rng), z), (R.rand_matrix(rng, log_h, 2), None, z[:1])]]
        _pin(p3, "%s width %d" % (hash, w), hash, kind, PROFILES[i % 2], (log_blowup, 0, 6, 2), log_h, rounds)


@pytest.mark.parametrize("hash,kind", HASHES)
def test_four_rounds_of_eight_matrices(p3, oracle, hash, kind):
    """PCS_MAX_ROUNDS x PCS_MAX_MATS: 32 matrices of widths 1..3, every one opened; the section order of the query openings over
    four trees of eight matrices and 60-odd pairs in pcs_ts_open_kernel / pcs_y_kernel."""
    rng = np.random.default_rng(48 + kind)
    z = [R.rand_point(rng) for _ in range(3)]
    rounds = [[(R.rand_matrix(rng, 4, 1 + (r + m) % 3), R.rand_shift(rng) if (r + m) % 2 else None, [z[(r + m) % 3]] + ([z[(r + m + 1) % 3]] if m % 3 == 0 else []))
               for m in range(8)] for r in range(4)]
    _pin(p3, hash, hash, kind, PROFILES[kind], (1, 1, 4, 3), 4, rounds)


def test_exactly_8192_batched_columns(p3, oracle):
    """PCS_MAX_COLS as an ACCEPTED open: one matrix 2048 wide at 4 points (the limit's comparison is `>`), 32 column tiles in the
    barycentric grid and an alpha-power table of 8192 entries."""
    rng = np.random.default_rng(8192)
    pts = [R.rand_point(rng) for _ in range(4)]
    rounds = [[(R.rand_matrix(rng, 3, 2048), R.rand_shift(rng), pts)]]
    opened = _pin(p3, "2048 x 4", "poseidon2", 0, "latency", (1, 0, 2, 2), 3, rounds)[0]
    assert len(opened) == 8192


def test_8193rd_batched_column_is_refused_by_open(p3, oracle):
    """the same limit as a refusal in Pcs::open, before anything touches the transcript"""
    rng = np.random.default_rng(8193)
    pts = [R.rand_point(rng) for _ in range(4)]
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(1, 0, 2, 2))
    _, d = pcs.commit([(R.rand_matrix(rng, 3, 2049), None)])
    ch = p3.Challenger()
    ch.observe(PREFIX)
    with pytest.raises(p3.P3HipError, match=r"round 0 matrix 0 point 3: more than 8192 batched columns \(sum of width over every \(matrix, point\) pair\)"):
        pcs.open([(d, [pts])], ch)
    fresh = p3.Challenger()
    fresh.observe(PREFIX)
    assert np.array_equal(ch.sample_ext(), fresh.sample_ext())
    d.free()
    pcs.free()


def _large_case(p3, hash, kind, t, log_h, rounds_dev, columns):
    """A shape too large for the reference prover.  rounds_dev = [[(device matrix, shift, points)]].  Asserts: the opened values of
    `columns` of every (matrix, point) pair equal pcs_ref.opened_value of those columns; the library's verifier and pcs_ref.verify
    accept and leave the prover's transcript; both reject a perturbed opened word."""
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
    datas = _commit_all(pcs, rounds_dev)
    ch = p3.Challenger(hash)
    ch.observe(PREFIX)
    opened, fri = _open(pcs, datas, rounds_dev, ch)
    k = 0
    for mats in rounds_dev:
        for m, s, pts in mats:
            w = m.shape[1]
            cols = sorted({c for c in columns if c < w} | {w - 1})
            sub = p3.host_u32(m[:, cols].contiguous())
            for z in pts:
                assert np.array_equal(opened[k:k + w][cols], R.opened_value(sub, R.ONE if s is None else s, z)), (k, w, cols)
                k += w
    assert k == len(opened)
    vr = [((root, [m.shape[1] for m, _, _ in mats]), [pts for _, _, pts in mats]) for (root, _), mats in zip(datas, rounds_dev)]

    def codes(op):
        c = p3.Challenger(hash)
        c.observe(PREFIX)
        ref = R.RefChallenger(kind)
        ref.observe(PREFIX)
        try:
            p3.pcs.verify(p3.FriParameters(*t), hash, vr, log_h, op, fri, c)
            lib = 0
        except p3.PcsRejected as e:
            lib = e.code
        return lib, R.verify(kind, t, log_h, vr, op, fri, ref), c, ref

    lib, ref, c, rc = codes(opened)
    assert (lib, ref) == (0, 0)
    nxt = ch.sample_ext()
    assert np.array_equal(c.sample_ext(), nxt) and np.array_equal(rc.sample_ext(), nxt)
    bad = opened.copy()
    bad[len(bad) // 2, 1] = (int(bad[len(bad) // 2, 1]) + 1) % P
    lib, ref, _, _ = codes(bad)
    assert lib != 0 and ref != 0
    for _, d in datas:
        d.free()
    pcs.free()


def test_uneven_barycentric_grid_at_2_15_rows(p3, oracle):
    """pcs_bary_kernel's grid min(1024, 4096 / tiles, h / (32 rps)) where it is no power of two: width 257 (5 tiles) gives 819
    blocks of per_blk = 41 rows, the last 19 of them with r_lo >= h; width 448 (7 tiles) gives 585 blocks of 57 rows.  A block that
    took per_blk = h / gridDim.x (rounded down) would leave rows out.  See _large_case for what is asserted."""
    import torch
    log_h = 15
    g = torch.Generator(device="cuda").manual_seed(257)
    rng = np.random.default_rng(257)
    z = [R.rand_point(rng) for _ in range(2)]
    mats = [torch.randint(0, P, (1 << log_h, w), dtype=torch.int32, device="cuda", generator=g) for w in (257, 448)]
    rounds = [[(mats[0], R.rand_shift(rng), z), (mats[1], None, z[1:])]]
    _large_case(p3, "poseidon2", 0, (1, 2, 3, 4), log_h, rounds, (0, 63, 64, 255, 256))


def test_narrow_and_wide_lde_plans_at_2_17_rows(p3, oracle):
    """2^17 rows, blowup 1: round 0 = widths 2 (random domain shift), 6, 16, round 1 = 20, 64; three distinct points, 4 queries.
    The first PCS run between 2^14 and 2^20 rows, on the narrow and the wide LDE plans of ntt_coset_lde with commit's GENERATOR / s
    shift, with 1024 barycentric blocks.  See _large_case for what is asserted."""
    import torch
    log_h = 17
    g = torch.Generator(device="cuda").manual_seed(17)
    rng = np.random.default_rng(17)
    z = [R.rand_point(rng) for _ in range(3)]
    mk = lambda w: torch.randint(0, P, (1 << log_h, w), dtype=torch.int32, device="cuda", generator=g)
    rounds = [[(mk(2), R.rand_shift(rng), [z[0], z[1]]), (mk(6), None, [z[2]]), (mk(16), None, [z[1]])],
              [(mk(20), None, [z[0]]), (mk(64), R.rand_shift(rng), [z[2], z[0]])]]
    _large_case(p3, "keccak", 1, (1, 0, 4, 5), log_h, rounds, (0, 63, 64, 255, 256))


# ---------------------------------------------------------------- values
AMPLITUDES = [0, 1, (P - 1) // 2, (P + 1) // 2, P - 1]


def _patterns(log_h):
    """20 columns: const, delta, alternating, block of structured_inputs at the five amplitudes (words)"""
    n, out = 1 << log_h, []
    for i, v in enumerate(AMPLITUDES):
        out += [S.const(log_h, v), S.delta(log_h, (0, 1, n // 2, n - 1, n // 3)[i], v), S.alternating(log_h, v, AMPLITUDES[(i + 2) % 5]),
                S.block(log_h, i % (log_h + 1), v)]
    return out


def _special_points(log_h, log_blowup, rng):
    a, b = (int(v) for v in R.O.to_monty(rng.integers(1, P, 2, dtype=np.uint64)))
    finer = R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_h + log_blowup + 1), 2 * int(rng.integers(0, 1 << (log_h + log_blowup))) + 1))
    e = lambda *w: np.array(w, dtype=np.uint32)
    return [[e(0, 0, 0, 0), R.ext_from_base(R.ONE), e(P - 1, 0, 0, 0), e(0, 1, 0, 0)],
            [e(a, 0, b, 0), e(0, a, 0, b), e(P - 1, P - 1, P - 1, P - 1), R.ext_from_base(finer)]]


@pytest.mark.parametrize("w", [2, 17, 64])
@pytest.mark.parametrize("log_h", [4, 6])
def test_structured_matrices_at_special_points(p3, oracle, log_h, w):
    """den_consts with z = 0, z1 = z3 = 0, z0 = z2 = 0 and P - 1 coordinates, base-field points 1, P - 1 (as a word) and one on the
    next finer coset GENERATOR g_(2 big)^odd; bb::dot2 in the barycentric and reduced-opening loops with 0 and P - 1 operands: the
    20 structured columns fill matrices of width w, every matrix opened at the four points of a group.  A dot2 that reduces
    a (P-1)(P-1) + (P-1)(P-1) sum one step short, or a den_consts that mistakes k0 for z = (a, 0, b, 0), changes the bytes."""
    cols = _patterns(log_h)
    n_mats = -(-len(cols) // w)
    for grp in range(2):
        hash, kind = HASHES[(grp + log_h // 4 + w) % 2]
        t = (1 + grp, 1, 4, 2)
        rng = np.random.default_rng(1000 * log_h + 10 * w + grp)
        pts = _special_points(log_h, t[0], rng)[grp]
        mats = [np.stack([cols[(m * w + c) % len(cols)] for c in range(w)], axis=1) for m in range(n_mats)]
        mats = [(m, R.rand_shift(rng) if i % 2 else None, pts) for i, m in enumerate(mats)]
        rounds = [mats[:8]] + ([mats[8:]] if len(mats) > 8 else [])
        _pin(p3, "%s log_h %d width %d group %d" % (hash, log_h, w, grp), hash, kind, PROFILES[grp], t, log_h, rounds)


@pytest.mark.parametrize("hash,kind", HASHES)
def test_constant_matrices_have_a_closed_form_proof(p3, oracle, hash, kind):
    """Every matrix constant: each opened value is (c, 0, 0, 0) word for word, every reduced opening vanishes, so commit-phase root
    r is oracle.mmcs_commit of the all-zero 2^(log_big - 1 - r) x 8 matrix and the final polynomial is zero.  Needs neither the
    reference prover nor the oracle's field arithmetic: an error common to the library and the restatements (a wrong barycentric
    factor, a Y - S that does not cancel) shows here."""
    rng = np.random.default_rng(60 + kind)
    for log_h, log_blowup, lfp in ((4, 1, 0), (6, 2, 2)):
        log_big = log_h + log_blowup
        pts = _special_points(log_h, log_blowup, rng)
        pts = [pts[0][0], pts[0][2], pts[1][2], R.rand_point(rng)]
        consts = [AMPLITUDES[(i + kind) % 5] for i in range(3)] + [int(rng.integers(0, P))]
        mats = [(np.full((1 << log_h, w), c, dtype=np.uint32), R.rand_shift(rng) if i % 2 else None, pts[i:] + pts[:i // 2])
                for i, (w, c) in enumerate(zip((2, 17, 64, 5), consts))]
        rounds = [mats[:2], mats[2:]]
        opened, fri, _, _ = _device(p3, hash, PROFILES[kind], (log_blowup, lfp, 3, 2), rounds)
        k = 0
        for (m, _, mp), c in zip(mats, consts):
            n = m.shape[1] * len(mp)
            assert np.array_equal(opened[k:k + n], np.tile(np.array([c, 0, 0, 0], dtype=np.uint32), (n, 1))), (log_h, c)
            k += n
        assert k == len(opened)
        words = np.frombuffer(fri, dtype=np.uint32)
        n_fr = log_h - lfp
        assert words[0] == n_fr
        for r in range(n_fr):
            zero_root, _ = oracle.mmcs_commit([np.zeros((1 << (log_big - 1 - r), 8), dtype=np.uint32)], kind)
            assert np.array_equal(words[1 + 8 * r:9 + 8 * r], zero_root), (log_h, r)
        fpl = 1 << lfp
        assert words[-2 - 4 * fpl] == fpl and not words[-1 - 4 * fpl:-1].any()


@pytest.mark.parametrize("w", [2, 17, 64])
def test_a_point_of_the_committed_domain_opens_to_a_row(p3, oracle, w):
    """Domain shift None and z = g_h^k: the point lies in the committed domain (and off the LDE coset), so the opened values are
    row k of the matrix, word for word, for k in {0, 1, h/2, h-1} (four points: pcs_bary_kernel<4>) with a random and an all-(P-1)
    matrix.  No reference arithmetic at all; a barycentric sum that loses or doubles one row fails it."""
    for i, (log_h, (hash, kind)) in enumerate(zip((3, 7), HASHES)):
        rng = np.random.default_rng(70 + w + i)
        h = 1 << log_h
        ks = [0, 1, h // 2, h - 1]
        pts = [R.ext_from_base(R.bpow(R.two_adic_generator(log_h), k)) for k in ks]
        mats = [R.rand_matrix(rng, log_h, w), np.full((h, w), P - 1, dtype=np.uint32)]
        opened, _, _, _ = _device(p3, hash, PROFILES[i], (1, 0, 2, 1), [[(m, None, pts) for m in mats]])
        want = np.zeros((2 * 4 * w, 4), dtype=np.uint32)
        want[:, 0] = np.concatenate([m[k] for m in mats for k in ks])
        assert np.array_equal(opened, want)


# ---------------------------------------------------------------- states
def _sequence(rng):
    """(log_h, [(width, points)]): shapes that grow, shrink, repeat with other data, change point counts and total columns"""
    z = [R.rand_point(rng) for _ in range(4)]
    shapes = [(3, [(3, z[:1])]), (6, [(17, z[:2]), (2, z[1:3])]), (9, [(40, z[:3])]), (3, [(3, z[1:2])]), (6, [(17, z[:1]), (2, z[2:4])]),
              (6, [(17, z[2:4]), (2, z[:2])]), (4, [(64, z), (65, [])]), (3, [(3, z[:1])]), (9, [(40, z[3:])]), (4, [(64, z[:1]), (65, z[:2])])]
    return [(log_h, [[(R.rand_matrix(rng, log_h, w), R.rand_shift(rng) if (i + j) % 2 else None, pts) for j, (w, pts) in enumerate(ms)]])
            for i, (log_h, ms) in enumerate(shapes)]


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("hash,kind", HASHES)
def test_one_object_through_changing_shapes(p3, oracle, hash, kind, own_stream):
    """Ten opens on one TwoAdicFriPcs: the arena rebuilt at every change of shape (`s.shape != shape`), kept when a shape repeats
    with other data, the scratch buffers of Impl::Buf that only grow (a smaller open after a larger one reads the front of a larger
    buffer).  Each result equals the reference prover's bytes (all shapes are small) and a fresh object's.  A reserve() that kept
    the old word count after a re-allocation, or an arena kept across a change of point counts, fails it."""
    t = (1, 1, 5, 3)
    seq = _sequence(np.random.default_rng(90))
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, own_stream=own_stream)
    for i, (log_h, rounds) in enumerate(seq):
        what = "%s open %d" % (hash, i)
        got = _pin(p3, what, hash, kind, "latency", t, log_h, rounds, key=("sequence", kind, i), pcs=pcs)
        if not own_stream:
            fresh = _device(p3, hash, "latency", t, rounds)
            assert got[1] == fresh[1] and np.array_equal(got[0], fresh[0]) and np.array_equal(got[3], fresh[3]), what
    pcs.free()


@pytest.mark.parametrize("hash,kind", HASHES)
def test_data_committed_by_one_object_opens_on_another(p3, oracle, hash, kind):
    """open's admission checks compare the PcsData's hash, device and blowup with the opening object's, not the object itself: a
    commitment of one object opens on a second of the same configuration (on its own stream, with another profile)."""
    t = (2, 0, 4, 2)
    rng = np.random.default_rng(95 + kind)
    z = [R.rand_point(rng) for _ in range(2)]
    rounds = [[(R.rand_matrix(rng, 5, 17), R.rand_shift(rng), z)], [(R.rand_matrix(rng, 5, 3), None, z[:1])]]
    a = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, "latency")
    b = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, "throughput", own_stream=True)
    datas = [a.commit([(m, s) for m, s, _ in rounds[0]]), b.commit([(m, s) for m, s, _ in rounds[1]])]
    ch = p3.Challenger(hash)
    ch.observe(PREFIX)
    opened, fri = _open(b, datas, rounds, ch)
    _equals_reference(hash, (opened, fri, [r for r, _ in datas], ch.sample_ext()), _reference(None, kind, t, 5, rounds))
    for _, d in datas:
        d.free()
    a.free()
    b.free()


def _tiny(rng):
    return [[(R.rand_matrix(rng, 3, 3), None, [R.rand_point(rng)])]]


def _handover(p3, hash, kind, states):
    """states = [(name, prepare)]: prepare(ch) brings a library Challenger or a RefChallenger (same methods) to the state"""
    t = (1, 0, 3, 4)
    rounds = _tiny(np.random.default_rng(97 + kind))
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
    for name, prepare in states:
        _pin(p3, "%s %s" % (hash, name), hash, kind, "latency", t, 3, rounds, pcs=pcs, prepare=prepare)
    pcs.free()


def _words(n, seed=0):
    return R.O.to_monty(np.arange(seed + 1, seed + n + 1, dtype=np.uint64) * 1000003 % P)


def test_poseidon2_challenger_handover(p3, oracle):
    """chal_to_dev / chal_from_dev for the duplex challenger: every n_in in 0..7 on a fresh state and on a permuted one, and every
    n_out in 1..7 (a partially drained output buffer, which the first observation of the open must clear).  A hand-over that
    dropped the pending inputs or kept the outputs alive changes alpha, hence every byte."""
    def pending(k, after_sample):
        def prepare(ch):
            if after_sample:
                ch.observe(_words(3, 50))
                ch.sample_ext()
            if k:
                ch.observe(_words(k, k))
        return prepare

    def drained(left):
        def prepare(ch):
            ch.observe(_words(11, 70))
            for _ in range(8 - left):
                ch.sample_bits(20)
        return prepare

    states = [("%d pending, fresh" % k, pending(k, False)) for k in range(8)]
    states += [("%d pending after a sample" % k, pending(k, True)) for k in range(1, 8)]
    states += [("%d outputs left" % m, drained(m)) for m in range(1, 8)]
    for m in range(1, 8):  # the states are what their names say
        ref = R.RefChallenger(0)
        drained(m)(ref)
        assert len(ref.out) == m and not ref.inb
    _handover(p3, "poseidon2", 0, states)


def test_keccak_challenger_handover(p3, oracle):
    """chal_to_dev for the hash challenger: keccak256_absorb_full consumes the complete 136-byte blocks of the pending input on the
    host and the rest becomes the device's partial block.  33 / 34 / 35 words are 132 / 136 / 140 bytes (below, exactly and above one
    block: blen = 0 at 34), 67 / 68 / 69 the same around two blocks, 100 words two blocks and 128 bytes; after a sample the 32-byte
    chaining value comes first, so 25 / 26 / 27 words make 132 / 136 / 140 bytes; 4, 16 and 28 output bytes left over, which the
    open's first observation discards.  A chal_to_dev that copied the pending bytes without absorbing full blocks overruns the
    136-byte block for every state from 136 bytes up; one that absorbed `>` instead of `>=` fails at exactly 34, 68 and 26."""
    def fresh(n):
        return lambda ch: ch.observe(_words(n, n))

    def after_sample(n):
        def prepare(ch):
            ch.observe(_words(4, 9))
            ch.sample_ext()
            ch.observe(_words(n, n))
        return prepare

    def left(want):
        def find():
            for seed in range(200):  # rejection sampling may take more bytes: the first prefix that leaves exactly `want`
                ref = R.RefChallenger(1)
                ref.observe(_words(5, seed))
                for _ in range((32 - want) // 4):
                    ref.sample_bits(16)
                if len(ref.obuf) == want:
                    return seed
            raise AssertionError(want)
        seed = find()

        def prepare(ch):
            ch.observe(_words(5, seed))
            for _ in range((32 - want) // 4):
                ch.sample_bits(16)
        return prepare

    states = [("%d words, fresh" % n, fresh(n)) for n in (33, 34, 35, 67, 68, 69, 100)]
    states += [("%d words after a sample" % n, after_sample(n)) for n in (25, 26, 27)]
    states += [("%d output bytes left" % b, left(b)) for b in (4, 16, 28)]
    for n, want in ((25, 132), (26, 136), (27, 140)):
        ref = R.RefChallenger(1)
        after_sample(n)(ref)
        assert len(ref.ibuf) == want
    _handover(p3, "keccak", 1, states)


@pytest.mark.parametrize("hash,kind", HASHES)
def test_a_challenger_that_came_back_from_an_open_enters_the_next(p3, oracle, hash, kind):
    """chal_from_dev then chal_to_dev: the Keccak challenger comes back with a sponge state that has absorbed blocks (`kst` nonzero) and
    a partial block; 40 more words take its pending input past a block boundary before the second open, so keccak256_absorb_full
    resumes from `kst`.  The reference challenger runs the same two opens.  A chal_to_dev that started from a zero sponge fails it."""
    t = (1, 0, 3, 4)
    rng = np.random.default_rng(98 + kind)
    cases = [_tiny(rng), [[(R.rand_matrix(rng, 4, 5), R.rand_shift(rng), [R.rand_point(rng)])]]]
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
    ch, ref = p3.Challenger(hash), R.RefChallenger(kind)
    for i, rounds in enumerate(cases):
        for c in (ch, ref):
            c.observe(_words(40, i))
        datas = _commit_all(pcs, rounds)
        opened, fri = _open(pcs, datas, rounds, ch)
        ropened, rfri, rroots = R.open_with_roots(kind, t, 3 + i, rounds, ref)
        assert np.array_equal(opened, ropened), i
        _same(fri, rfri, "%s open %d" % (hash, i))
        c2 = ch.clone()  # a clone carries the absorbed blocks too
        assert np.array_equal(c2.sample_ext(), ref.clone().sample_ext()), i
        for _, d in datas:
            d.free()
    assert np.array_equal(ch.sample_ext(), ref.sample_ext())
    pcs.free()


def test_evaluations_on_domain_of_a_later_matrix_with_a_shift(p3, oracle):
    """get_evaluations_on_domain (p3hip_pcs_lde_dev) for matrix index >= 1 committed with a domain shift, at every log_size from
    log_h to log_big: the first 2^log_size rows of oracle.coset_lde_batch with shift GENERATOR / s, bit-reversed."""
    rng = np.random.default_rng(99)
    log_h, log_blowup = 5, 3
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(log_blowup, 0, 2, 1))
    ms = [(R.rand_matrix(rng, log_h, w), R.rand_shift(rng)) for w in (3, 17, 64)]
    _, d = pcs.commit(ms)
    for i in (1, 2):
        m, s = ms[i]
        lde = oracle.coset_lde_batch(m, log_blowup, R.bmul(R.GEN, R.binv(s)), bit_reversed_out=True)
        for log_size in range(log_h, log_h + log_blowup + 1):
            got = pcs.get_evaluations_on_domain(d, i, log_size)
            assert tuple(got.shape) == (1 << log_size, m.shape[1])
            assert np.array_equal(p3.host_u32(got), lde[:1 << log_size]), (i, log_size)
    d.free()
    pcs.free()
