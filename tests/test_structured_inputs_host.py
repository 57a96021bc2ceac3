"""CPU tests of tests/structured_inputs.py (the generators and closed forms the GPU tests of extreme and structured inputs
rest on) and of the ORACLE on the same inputs: generator properties by plain integer arithmetic, closed forms against the
big-int pyref and against the oracle's coset LDE, and the degenerate proof instances through the oracle's provers and
verifiers and the product's host verifiers."""
import numpy as np
import pytest

import pyref
import structured_inputs as si

P = si.P
GEN_MONTY = si.to_word(31)
ONE_MONTY = si.to_word(1)


def _split(log_h):
    n1 = (log_h + 1) // 2  # the narrow plan's digits: n = n1 + n2, n1 = ceil(n / 2) (ntt.hip lde_narrow)
    return n1, log_h - n1


# ---------------------------------------------------------------- generator properties
@pytest.mark.parametrize("log_h", range(16, 25))
def test_block_and_const_fill_the_first_digit_tiles(log_h):
    """Row i = r1 N2 + r2.  K1 sums over r1 for every r2: const(P-1) makes every such tile all P-1 (integer sum 2^n1 (P-1),
    against about 2^(n1-1) P for uniform words), and block(n2, P-1) leaves the WORD P-1 as every column sum, so that K2's
    k1 = 0 tile (the 2^n2 sums over r1, one per r2) is all P-1."""
    n1, n2 = _split(log_h)
    x = si.block(log_h, n2, P - 1).reshape(1 << n1, 1 << n2).astype(np.uint64)
    sums = x.sum(axis=0)
    assert sums.shape == (1 << n2,) and (sums == P - 1).all()
    c = si.const(log_h, P - 1).reshape(1 << n1, 1 << n2).astype(np.uint64)
    assert (c.sum(axis=0) == (P - 1) << n1).all()
    rng = np.random.default_rng(log_h)
    u = rng.integers(0, P, size=(1 << n1, 1 << min(n2, 8)), dtype=np.uint64).sum(axis=0)
    assert u.max() < ((P - 1) << n1) * 0.6  # what uniform words reach: about half, never the same binade's top


@pytest.mark.parametrize("log_h", range(16, 25))
def test_coefficient_families_scale_to_the_intended_words(log_h):
    """coeff_block(n1, ..) / coeff_comb(n1, ..): c[k] (shift g^j)^k, recomputed by MULTIPLICATION with Python pow, is v on the
    block / comb and c is zero elsewhere.  k = k1 + N1 k2: the block is k2 = 0 (K3's tile of m2 = 0 reads v for every k1),
    the comb is k1 = 0 (K2's forward digit of k1 = 0 reads v for every k2)."""
    n1, n2 = _split(log_h)
    rng = np.random.default_rng(100 + log_h)
    for added, shift, v in [(1, GEN_MONTY, P - 1), (2, int(rng.integers(1, P)), (P + 1) // 2), (3, ONE_MONTY, (P - 1) // 2)]:
        g = si.two_adic_generator(log_h + added)
        for j in (0, (1 << added) - 1):
            t = si.from_word(shift) * pow(g, j, P) % P
            for fam, ks in (("coeff_block", range(1 << n1)), ("coeff_comb", range(0, 1 << log_h, 1 << n1))):
                c = si.generate(fam, log_h, m=n1, v=v, shift=shift, j=j, added=added)
                assert c.dtype == np.uint32 and c.shape == (1 << log_h,) and int(c.max()) < P
                ks = list(ks)
                assert np.count_nonzero(c) == len(ks)  # zero off the set (v != 0 and the scale is a unit)
                assert all(int(c[k]) * pow(t, k, P) % P == v for k in ks), (fam, added, j)


def test_eval_generators_shapes_and_values():
    rng = np.random.default_rng(1)
    for log_h in range(0, 7):
        n = 1 << log_h
        assert si.const(log_h, 5).tolist() == [5] * n
        for r in si.delta_rows(log_h, rng):
            assert si.delta(log_h, r, 9).tolist() == [9 if i == r else 0 for i in range(n)]
        assert si.alternating(log_h, 3, 4).tolist() == [3 if i % 2 == 0 else 4 for i in range(n)]
        for m in range(log_h + 1):
            assert si.block(log_h, m, 7).tolist() == [7 if i < (1 << m) else 0 for i in range(n)]
            assert si.comb(log_h, m, 7).tolist() == [7 if i % (1 << m) == 0 else 0 for i in range(n)]
    cols = [si.const(4, 1), si.const(4, 2)]
    mat, pos = si.pack(cols, 5, np.random.default_rng(2))
    assert mat.shape == (16, 5) and len(pos) == 2 and int(mat.max()) < P
    assert all((mat[:, p] == c).all() for p, c in zip(pos, cols))
    a = np.arange(1, 2000, dtype=np.uint64)
    assert ((si.batch_inverse(a) * a) % np.uint64(P) == 1).all()
    assert si.geometric(3, 5).tolist() == [1, 3, 9, 27, 81]


# ---------------------------------------------------------------- closed forms against big-int pyref
def _shifts(rng):
    return [GEN_MONTY, ONE_MONTY, int(rng.integers(1, P))]


@pytest.mark.parametrize("log_h", range(0, 6))
def test_closed_forms_against_pyref(log_h):
    rng = np.random.default_rng(7 + log_h)
    n = 1 << log_h
    for added in (0, 1, 2):
        rows = list(range(n << added))
        for shift in _shifts(rng):
            for fam, prm in si.family_cases(log_h, added, shift, rng, ampl=si.AMPL, coeff_ampl=si.AMPL):
                col = [int(v) for v in si.column_of(fam, prm)]
                if fam in si.COEFF_FAMILIES:
                    col = pyref.naive_dft_col(col)  # the evaluation-domain input of a coefficient family
                exp = [r[0] for r in pyref.coset_lde([[v] for v in col], added, si.from_word(shift))]
                assert si.closed_form(fam, prm, rows).tolist() == exp, (fam, prm)


# ---------------------------------------------------------------- closed forms against the oracle
def _check_against_oracle(oracle, cases, log_h, added, shift, rows, width=None):
    """packs the cases' columns (16 per matrix), runs the oracle's natural-order LDE and compares the closed forms at `rows`"""
    rng = np.random.default_rng(log_h * 31 + added)
    per = width or 16
    for k0 in range(0, len(cases), per):
        part = cases[k0:k0 + per]
        cols = []
        for fam, prm in part:
            c = si.column_of(fam, prm)
            cols.append(oracle.dft_batch(c.reshape(-1, 1)).reshape(-1) if fam in si.COEFF_FAMILIES else c)
        mat, pos = si.pack(cols, max(len(cols), width or 0) + (0 if width else 1), rng)
        out = oracle.coset_lde_batch(mat, added, shift)
        for (fam, prm), p in zip(part, pos):
            exp = si.closed_form(fam, prm, rows)
            got = out[rows, p]
            assert np.array_equal(got, exp), (fam, prm, [int(rows[i]) for i in np.nonzero(got != exp)[0][:4]])


@pytest.mark.parametrize("log_h", range(0, 13))
def test_closed_forms_against_oracle_every_row(oracle, log_h):
    rng = np.random.default_rng(50 + log_h)
    shifts = _shifts(rng)
    if log_h <= 6:  # every blowup with every shift, every amplitude
        configs, ampl = [(a, s) for a in (0, 1, 2) for s in shifts], si.AMPL
    elif log_h <= 9:
        configs, ampl = list(zip((0, 1, 2), shifts)), (P - 1,)
    else:  # one configuration per height: the closed forms cost a few Python pows per row and column
        configs, ampl = [(log_h % 3, shifts[log_h % 3])], (P - 1,)
    for added, shift in configs:
        cases = si.family_cases(log_h, added, shift, rng, ampl=ampl, coeff_ampl=ampl)
        _check_against_oracle(oracle, cases, log_h, added, shift, np.arange((1 << log_h) << added))


@pytest.mark.parametrize("log_h,added", [(16, 1), (16, 2), (16, 3)])
def test_closed_forms_against_oracle_2_16(oracle, log_h, added):
    """every family, the full m sweep, at 2^16 rows; 256 seeded rows plus 0, 1, n-1, n and the last"""
    rng = np.random.default_rng(160 + added)
    shift = GEN_MONTY if added == 1 else int(rng.integers(1, P))
    rows = np.array(si.sample_rows(log_h, added, rng, 256))
    cases = si.family_cases(log_h, added, shift, rng, coeff_ampl=(P - 1, (P + 1) // 2) if added == 1 else ((P - 1) // 2,))
    oracle.set_threads(oracle.test_threads())
    try:
        _check_against_oracle(oracle, cases, log_h, added, shift, rows)
    finally:
        oracle.set_threads(1)


def test_closed_forms_against_oracle_2_20_x_2(oracle):
    """The headline shape, 2^20 x 2 at blowup 2: const, block(n2) and coeff_block(n1) at P-1 (and 2^19 x 16, 2^16 x 2 for
    coeff_block(8, P-1)): the oracle agrees with the closed forms where its own sums are the largest."""
    rng = np.random.default_rng(200)
    oracle.set_threads(oracle.test_threads())
    try:
        for log_h, width, shift in [(20, 2, GEN_MONTY), (19, 16, GEN_MONTY), (16, 2, int(rng.integers(1, P)))]:
            n1, n2 = _split(log_h)
            base = {"log_h": log_h, "added": 1, "shift": shift}
            cases = [("const", dict(base, v=P - 1)), ("block", dict(base, m=n2, v=P - 1)),
                     ("coeff_block", dict(base, m=n1, v=P - 1, j=0)), ("coeff_block", dict(base, m=n1, v=P - 1, j=1)),
                     ("coeff_block", dict(base, m=8, v=P - 1, j=1)), ("coeff_comb", dict(base, m=n1, v=(P + 1) // 2, j=1))]
            rows = np.array(si.sample_rows(log_h, 1, rng, 256))
            _check_against_oracle(oracle, cases, log_h, 1, shift, rows, width=width)
    finally:
        oracle.set_threads(1)


# ---------------------------------------------------------------- degenerate proof instances
DEGENERATE = [(0, 0), (P, 2 * P), (2 ** 64 - 1, 2 ** 64 - 1), (P - 1, P - 1), (P - 1, 1)]
T = (1, 0, 10, 4)


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
@pytest.mark.parametrize("log_n", [1, 3, 10])
def test_degenerate_instances_oracle_and_host_verifiers(p3, oracle, log_n, hash_name, hiding):
    """(0, 0) — a zero trace, zero quotient, zero FRI layers — and unreduced a, b up to 2^64 - 1 (legal at the C ABI, reduced by
    the libraries): the oracle proves, its verifier and the product's host verifier accept, a wrong x is rejected by both, and
    (P, 2P) gives the bytes of (0, 0)."""
    kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
    ofp, gfp = oracle.FriParams(*T), p3.FriParameters(*T)
    prove = (lambda a, b: oracle.prove_fib_air_hiding(a, b, log_n, ofp, hash=kind, seed=1)) if hiding else \
            (lambda a, b: oracle.prove_fib_air(a, b, log_n, ofp, hash=kind))
    overify = oracle.verify_fib_air_hiding if hiding else oracle.verify_fib_air
    proofs = {}
    for a, b in DEGENERATE:
        proof = proofs[(a, b)] = prove(a, b)
        x = oracle.fib_public_x(a, b, 1 << log_n)
        assert x == p3.fib_public_x(a, b, 1 << log_n)
        assert overify(proof, a, b, x, log_n, ofp, hash=kind) == 0, (a, b)
        assert overify(proof, a % P, b % P, x, log_n, ofp, hash=kind) == 0, (a, b)  # the statement is the reduced one
        p3.verify_fib_air(proof, a, b, x, log_n, gfp, hash=hash_name, hiding=hiding)  # accepts
        assert overify(proof, a, b, (x + 1) % P, log_n, ofp, hash=kind) != 0, (a, b)
        with pytest.raises(p3.P3HipError):
            p3.verify_fib_air(proof, a, b, (x + 1) % P, log_n, gfp, hash=hash_name, hiding=hiding)
    assert proofs[(P, 2 * P)] == proofs[(0, 0)]
    assert proofs[(P - 1, P - 1)] != proofs[(0, 0)]
    assert oracle.fib_public_x(0, 0, 1 << log_n) == 0
