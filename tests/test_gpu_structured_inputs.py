"""GPU tests (MI355X) on EXTREME and STRUCTURED values: constant, delta, alternating, block and comb columns at the amplitude
words P-1, 1, (P-1)/2, (P+1)/2 and 0, and coefficient columns whose scaled coefficients are such blocks and combs
(tests/structured_inputs.py).  Every other GPU test of the transforms feeds them uniformly random words, whose butterfly sums
stay near half the worst case and whose results are ~never 0; these inputs put all-equal extreme tiles into every digit of the
narrow plan (K1, K2 inverse, K2 forward, K3: tests/test_structured_inputs_host.py states which input fills which tile) and make
zeros and equal operands the norm in every butterfly.

Everything is bit-exact against the oracle, and the closed form of the output is asserted as well at sampled rows, so that a
failure names which of the two the GPU disagrees with.  Trees and proofs: all-P-1, all-zero and alternating matrices layer by
layer, and the degenerate instances (0, 0), unreduced a, b >= P up to 2^64 - 1, (P-1, P-1), (P-1, 1) byte for byte."""
import functools

import numpy as np
import pytest

import structured_inputs as si

pytestmark = pytest.mark.gpu
P = si.P
CENTRED = ((P - 1) // 2, (P + 1) // 2)


@pytest.fixture(scope="module")
def dft(p3):
    ok, msg = p3.is_available()
    assert ok, msg
    return p3.GpuDft.with_backend(p3.BackendKind.Hip)


class _threads:
    """the oracle on the host's cores for the large calls (serial otherwise, like every other test)"""

    def __init__(self, oracle):
        self.o = oracle

    def __enter__(self):
        self.o.set_threads(self.o.test_threads())

    def __exit__(self, *exc):
        self.o.set_threads(1)


def _split(log_h):
    n1 = (log_h + 1) // 2  # ntt.hip lde_narrow: n = n1 + n2, n1 = ceil(n / 2)
    return n1, log_h - n1


def _special_ms(log_h):
    n1, n2 = _split(log_h)
    return (0, 1, n2 - 1, n2, n2 + 1, n1, log_h - 1, log_h)


def _describe(case):
    fam, prm = case
    return "%s(%s)" % (fam, ", ".join("%s=%s" % (k, prm[k]) for k in ("m", "r", "v", "u", "j") if k in prm))


def _check(got, exp, cases, pos, col0, log_h, added, rows, brev, closed, what):
    """got / exp: one GPU call's output and the oracle's columns for it; cases[k] sits in column pos[k] - col0 where that lies
    inside this slice.  Bit-exact against the oracle first (the message names the column's family, the natural-order row and
    whom the closed form sides with), then the closed forms at the sampled rows."""
    bits = log_h + added
    mine = [(c, p - col0, cf) for c, p, cf in zip(cases, pos, closed) if 0 <= p - col0 < got.shape[1]]
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        r, c = (int(v) for v in np.argwhere(got != exp)[0])
        nat = int(si.bit_reverse_index([r], bits)[0]) if brev else r
        case = next((cs for cs, p, _ in mine if p == c), None)
        side = "a random fill column"
        if case is not None:
            cf = int(si.closed_form(case[0], case[1], [nat])[0])
            side = "%s; the closed form (%d) sides with %s" % (
                _describe(case), cf, "the ORACLE (kernel bug)" if cf == int(exp[r, c]) else
                "the GPU (oracle bug)" if cf == int(got[r, c]) else "neither")
        pytest.fail("%s: 2^%d rows, blowup 2^%d: %d words differ from the oracle, first at natural row %d, column %d: gpu %d, "
                    "oracle %d; %s" % (what, log_h, added, int((got != exp).sum()), nat, c, int(got[r, c]), int(exp[r, c]), side))
    idx = si.bit_reverse_index(rows, bits) if brev else np.asarray(rows)
    for case, p, cf in mine:
        assert np.array_equal(got[idx, p], cf), (what, "closed form", _describe(case), log_h, added)


def _lde_batch(dft, oracle, p3, cases, widths, added, shift, rng, brev=True, host_slice=None, from_coeffs=False, n_rows=6):
    """One oracle LDE over sum(widths) columns (the patterns at seeded positions, seeded random words in the rest), and one GPU
    LDE per slice of widths[k] columns through the device entry point (slice `host_slice` also through the host-pointer one).
    from_coeffs: all cases are coefficient families; they are packed as COEFFICIENTS, the evaluation-domain input is the oracle's
    dft of that matrix, and every slice also goes through p3hip_coset_lde_from_coeffs_bb31_dev."""
    log_h = cases[0][1]["log_h"]
    total = sum(widths)
    assert len(cases) <= total
    if from_coeffs:
        assert all(f in si.COEFF_FAMILIES for f, _ in cases)
        cmat, pos = si.pack([si.column_of(f, p) for f, p in cases], total, rng)
        x = oracle.dft_batch(cmat)
    else:
        cols = [si.column_of(f, p) for f, p in cases]
        ci = [k for k, (f, _) in enumerate(cases) if f in si.COEFF_FAMILIES]
        if ci:
            ev = oracle.dft_batch(np.stack([cols[k] for k in ci], axis=1))
            for t, k in enumerate(ci):
                cols[k] = ev[:, t]
        x, pos = si.pack(cols, total, rng)
    exp = oracle.coset_lde_batch(x, added, shift, brev)
    rows = si.sample_rows(log_h, added, rng, n_rows)
    closed = [si.closed_form(f, p, rows) for f, p in cases]
    col0 = 0
    for k, w in enumerate(widths):
        sl = slice(col0, col0 + w)
        xs, es = np.ascontiguousarray(x[:, sl]), exp[:, sl]
        args = (es, cases, pos, col0, log_h, added, rows, brev, closed)
        got = p3.host_u32(dft.coset_lde_batch(p3.dev_u32(xs), added, shift, bit_reversed_out=brev))
        _check(got, *args, "coset_lde _dev W=%d" % w)
        if k == host_slice:
            _check(dft.coset_lde_batch(xs, added, shift, bit_reversed_out=brev), *args, "coset_lde host entry W=%d" % w)
        if from_coeffs:
            assert brev
            got = p3.host_u32(p3.coset_lde_from_coeffs(p3.dev_u32(np.ascontiguousarray(cmat[:, sl])), added, shift))
            _check(got, *args, "coset_lde_from_coeffs W=%d" % w)
        col0 += w


def _sweep(dft, oracle, p3, log_h, templates, widths, addeds, shifts, rng, from_coeffs=False, spare=None, host_first=True):
    """templates -> batches of sum(widths) - spare columns (spare: random fill columns per batch, default one per slice);
    batch k runs at blowup addeds[k % ..] and shift shifts[k % ..]."""
    spare = len(widths) if spare is None else spare
    per = sum(widths) - spare
    for k, t0 in enumerate(range(0, len(templates), per)):
        added, shift = addeds[k % len(addeds)], shifts[k % len(shifts)]
        cases = [si.bind(t, log_h, added, shift) for t in templates[t0:t0 + per]]
        _lde_batch(dft, oracle, p3, cases, widths, added, shift, rng, host_slice=(k % len(widths)) if host_first and k == 0 else None,
                   from_coeffs=from_coeffs)


def _f64_templates(log_h, rng):
    """A's inputs: the full m sweep of all four block / comb families at P-1, const at every amplitude and 0, the deltas (every
    amplitude in turn), alternating; the coefficient families also on coset 0 and at the centred amplitudes at the m that matter
    to some digit (0, n2, n1, log_h), coeff_comb at the centred amplitudes at every other m too."""
    n1, n2 = _split(log_h)
    special = (0, n2, n1, log_h)
    ev = si.eval_templates(log_h, rng, delta_ampl=tuple(si.AMPL))
    co = si.coeff_templates(log_h, None, (P - 1,), ("last",)) + si.coeff_templates(log_h, special, (P - 1,), ("first",)) + \
        si.coeff_templates(log_h, special, CENTRED, ("last",))
    # K2's forward digit reads products, i.e. centred values: its all-equal tile of the largest magnitude is a comb at (P+-1)/2
    done = {(f, t["m"], t["v"]) for f, t in co}
    co += [t for t in si.coeff_templates(log_h, None, CENTRED, ("first",)) if t[0] == "coeff_comb" and (t[0], t[1]["m"], t[1]["v"]) not in done]
    return ev, co


# ---------------------------------------------------------------- A. narrow plan, fp64 butterflies
@pytest.mark.parametrize("log_h", [16, 17, 18, 19])
def test_narrow_f64_extreme_tiles(dft, oracle, p3, log_h):
    """2^16 .. 2^19 rows x W in {2, 4, 6, 8, 16}, blowup 2 / 4 / 8, bit-reversed output: the fp64 three-launch LDE, whose x + y
    half of every butterfly is unreduced for a whole digit (ntt_narrow_f64.hip.h).  const(P-1) makes every K1 tile all P-1 (sum
    2^n1 (P-1); uniform words reach about 2^(n1-1) P), block(n2, P-1) the k1 = 0 tile of K2's inverse digit, coeff_comb(n1, ..)
    the k1 = 0 tile of K2's forward digit (all-equal centred products of the largest magnitude at (P+-1)/2), coeff_block(n1, P-1)
    K3's tile of m2 = 0 on the chosen coset; the sweep over every m keeps that true whatever the digit split becomes."""
    rng = np.random.default_rng(1600 + log_h)
    ev, co = _f64_templates(log_h, rng)
    # shift 1 among them: the LDE then passes through the input's own rows, so results that are exactly 0 fill the output
    shifts = [p3.MONTY_ONE, p3.GENERATOR_MONTY, int(rng.integers(1, P))]
    with _threads(oracle):
        _sweep(dft, oracle, p3, log_h, ev, [2, 4, 6, 8, 16], (1, 2, 3), shifts, rng)
        _sweep(dft, oracle, p3, log_h, co, [16, 8, 6, 4, 2], (2, 1, 3), shifts[::-1], rng, from_coeffs=True, host_first=False)


def test_narrow_f64_extreme_tiles_headline_2_20_x_2(dft, oracle, p3):
    """2^20 x 2, the trace LDE of the headline proof: 10-stage fp64 digits, sums up to 2^10 (P-1).  Mostly at its own blowup 2,
    every eighth pair of batches at 4 / 8; the oracle extends 16 columns at a time, the GPU one column pair at a time."""
    log_h = 20
    rng = np.random.default_rng(2002)
    ev, co = _f64_templates(log_h, rng)
    shifts = [p3.GENERATOR_MONTY, p3.MONTY_ONE, p3.GENERATOR_MONTY, int(rng.integers(1, P))]
    with _threads(oracle):
        _sweep(dft, oracle, p3, log_h, ev, [2] * 8, (1, 1, 1, 2), shifts, rng, spare=1)
        _sweep(dft, oracle, p3, log_h, co, [2] * 8, (1, 1, 3, 1), shifts, rng, from_coeffs=True, spare=1, host_first=False)


# ---------------------------------------------------------------- B. narrow plan, integer butterflies; the wide form
def _int_templates(log_h, rng, ms, centred=False):
    ev = si.eval_templates(log_h, rng, ms, const_ampl=(P - 1, 0), delta_ampl=tuple(si.AMPL))
    co = si.coeff_templates(log_h, ms, (P - 1,), ("last",))
    if centred:
        co += si.coeff_templates(log_h, ms, CENTRED, ("first",))
    return ev + co


@pytest.mark.parametrize("log_h,widths,added,ms", [
    (20, [4, 16, 4, 16, 4], 1, None), (21, [8, 16, 8, 16], 1, None), (22, [4, 8, 16, 16], 1, None), (24, [2, 2], 2, "one"),
    (16, [65], 2, None), (17, [100], 1, None), (18, [64], 2, None)])
def test_narrow_integer_and_wide_plans(dft, oracle, p3, log_h, widths, added, ms):
    """The integer three-launch kernels (2^20 x 4 / 16, 2^21, 2^22, and 2^24 x 2 at blowup 4: cfg3's own shape, blocked
    intermediates and the out-of-place K3) and the wide form (2^16 x 65, 2^17 x 100, 2^18 x 64).  They reduce at every butterfly
    (bb31.hip.h: the branch-free min() corrections, the a - b + P operand), so the corner is results that are = 0 and equal
    operands, which these inputs make the norm; m in {0, 1, n2-1, n2, n2+1, n1, log_h-1, log_h}; at 2^24 (the
    oracle's cost) the four all-equal-tile inputs only: const(P-1), block(n2, P-1), coeff_block(n1, P-1), coeff_comb(n1, (P+1)/2)."""
    rng = np.random.default_rng(2400 + 10 * log_h + len(widths))
    n1, n2 = _split(log_h)
    shift = p3.GENERATOR_MONTY if log_h % 2 == 0 else int(rng.integers(1, P))
    if ms == "one":
        tmpl = [("const", {"v": P - 1}), ("block", {"m": n2, "v": P - 1}), ("coeff_block", {"m": n1, "v": P - 1, "j": "last"}),
                ("coeff_comb", {"m": n1, "v": (P + 1) // 2, "j": "first"})]
    else:
        tmpl = _int_templates(log_h, rng, _special_ms(log_h), centred=widths[0] > 64)
    with _threads(oracle):
        _sweep(dft, oracle, p3, log_h, tmpl, widths, (added,), (shift,), rng, spare=0 if ms == "one" else 1, host_first=log_h < 22)


# ---------------------------------------------------------------- C. general and fast plans
@pytest.mark.parametrize("log_h", list(range(0, 16)) + [16, 17])
def test_general_and_fast_plans(dft, oracle, p3, log_h):
    """dft_batch, idft_batch, coset_dft_batch and the natural-order coset_lde_batch at every height 2^0 .. 2^15, 2^16, 2^17 and
    widths 1, 2, 3, 8, 33 on every evaluation family with the full m sweep: against the oracle, against the closed forms, and
    against identities that need neither: dft(const v) is n v at row 0 and zero elsewhere, dft(delta(r, v)) is the geometric
    sequence v w^(r k), idft returns the input, and at shift 1 every 2^added-th row of the LDE is the input."""
    rng = np.random.default_rng(300 + log_h)
    n = 1 << log_h
    widths = [1, 2, 3, 8, 33]
    tmpl = si.eval_templates(log_h, rng, delta_ampl=tuple(si.AMPL))
    per = sum(widths) - len(widths)
    w_n = si.two_adic_generator(log_h)
    with _threads(oracle):
        for k, t0 in enumerate(range(0, len(tmpl), per)):
            added = (log_h + k) % 4
            shift = p3.GENERATOR_MONTY if (log_h + k) % 2 == 0 else int(rng.integers(1, P))
            cases = [si.bind(t, log_h, added, shift) for t in tmpl[t0:t0 + per]]
            x, pos = si.pack([si.column_of(f, p) for f, p in cases], sum(widths), rng)
            e_dft, e_cdft = oracle.dft_batch(x), oracle.coset_dft_batch(oracle.idft_batch(x), shift)
            e_lde = oracle.coset_lde_batch(x, added, shift)
            rows = si.sample_rows(log_h, added, rng, 6)
            closed = [si.closed_form(f, p, rows) for f, p in cases]
            for (f, prm), p in zip(cases, pos):  # the oracle's dft against the identities first: they judge it too
                if f == "const":
                    assert int(e_dft[0, p]) == n * prm["v"] % P and not e_dft[1:, p].any(), ("oracle dft(const)", log_h, prm)
                elif f == "delta":
                    geo = si.geometric(pow(w_n, prm["r"], P), n) * np.uint64(prm["v"]) % np.uint64(P)
                    assert np.array_equal(e_dft[:, p], geo.astype(np.uint32)), ("oracle dft(delta)", log_h, prm)
            col0 = 0
            for s, w in enumerate(widths):
                sl = slice(col0, col0 + w)
                xs = np.ascontiguousarray(x[:, sl])
                dev = (s + log_h + k) % 2 == 0  # device entry points and host-pointer ones in turn
                put = p3.dev_u32 if dev else (lambda a: a)
                get = p3.host_u32 if dev else (lambda a: a)
                what = "2^%d x %d (%s entry)" % (log_h, w, "device" if dev else "host")
                g_dft = get(dft.dft_batch(put(xs)))
                assert np.array_equal(g_dft, e_dft[:, sl]), ("dft_batch", what)
                assert np.array_equal(get(dft.idft_batch(put(g_dft))), xs), ("idft_batch(dft_batch)", what)
                coeffs = get(dft.idft_batch(put(xs)))
                assert np.array_equal(get(dft.coset_dft_batch(put(coeffs), shift)), e_cdft[:, sl]), ("coset_dft_batch", what)
                g_lde = get(dft.coset_lde_batch(put(xs), added, shift))
                _check(g_lde, e_lde[:, sl], cases, pos, col0, log_h, added, rows, False, closed, "natural-order coset_lde " + what)
                g_one = get(dft.coset_lde_batch(put(xs), added, p3.MONTY_ONE))
                assert np.array_equal(g_one[::1 << added], xs), ("shift 1: the LDE extends the input itself", what, added)
                col0 += w


@pytest.mark.parametrize("log_h", [22, 24])
def test_large_heights_const_and_block_on_the_device(dft, p3, log_h):
    """2^22 and 2^24 rows x 2 on the device, const(P-1) next to block(log_h / 2, P-1): no oracle run; the round trip, the dft's
    closed forms (n v at row 0 and zeros; v (w^(k L) - 1) / (w^k - 1) for the block of L rows) and the LDE's closed forms at
    sampled rows, natural order (general plan) and bit-reversed (the narrow plan's integer kernels)."""
    import torch
    n, m = 1 << log_h, log_h // 2
    rng = np.random.default_rng(log_h)
    xd = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    xd[:, 0] = P - 1
    xd[:1 << m, 1] = P - 1
    yd = dft.dft_batch(xd)
    assert torch.equal(dft.idft_batch(yd), xd)
    ks = sorted({0, 1, 2, n // 2, n - 1} | {int(v) for v in rng.integers(0, n, size=64)})
    got = p3.host_u32(yd[torch.tensor(ks, device="cuda")])
    w = si.two_adic_generator(log_h)
    assert int(got[0, 0]) == n * (P - 1) % P and not bool(yd[1:, 0].any())
    assert got[:, 1].tolist() == [(P - 1) * si._geom_sum(pow(w, k, P), 1 << m) % P for k in ks]
    del yd
    shift = p3.GENERATOR_MONTY
    base = {"log_h": log_h, "added": 1, "shift": shift, "v": P - 1}
    rows = si.sample_rows(log_h, 1, rng, 64)
    exp = np.stack([si.closed_form("const", base, rows), si.closed_form("block", dict(base, m=m), rows)], axis=1)
    for brev in (False, True):
        lde = dft.coset_lde_batch(xd, 1, shift, bit_reversed_out=brev)
        idx = si.bit_reverse_index(rows, log_h + 1) if brev else np.asarray(rows)
        assert np.array_equal(p3.host_u32(lde[torch.from_numpy(idx).cuda()]), exp), (log_h, "bit-reversed" if brev else "natural")
        if not brev:
            ext = dft.coset_lde_batch(xd, 1, p3.MONTY_ONE)
            assert torch.equal(ext[::2], xd)
            del ext
        del lde


# ---------------------------------------------------------------- D. trees
LEAF_WIDTHS = [1, 7, 8, 9, 16, 17, 64, 2633]


def _tree_matrix(kind, h, w):
    if kind == "all P-1":
        return np.full((h, w), P - 1, dtype=np.uint32)
    if kind == "all 0":
        return np.zeros((h, w), dtype=np.uint32)
    m = np.zeros((h, w), dtype=np.uint32)  # alternating rows: P-1 rows and zero rows, and the two words in turn inside a row
    m[::2, ::2] = P - 1
    m[1::2, 1::2] = P - 1
    return m


def _tree_shapes():
    """every leaf width at every height 2^0 .. 2^15 that keeps a matrix within 2^19 words (the oracle's sponge is the cost),
    and the widest row once more at 2^11"""
    out = [(1 << lh, w) for lh in range(16) for w in LEAF_WIDTHS if (w << lh) <= 1 << 19]
    return out + [(1 << 11, 2633)]


@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
def test_trees_over_extreme_matrices(p3, oracle, hash_name):
    """The sponge fed raw P-1 words (the fp64 form of the permutation converts them unreduced), zeros and their alternation:
    leaf widths 1 .. 2633 at heights 2^0 .. 2^15, under both thread profiles; the root and EVERY digest layer against
    oracle.Tree, three openings each checked by the oracle's verify_batch; one mixed-height commitment with injected matrices."""
    kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
    rng = np.random.default_rng(44)
    sets = [([(h, w)], what) for h, w in _tree_shapes() for what in ("all P-1", "all 0", "alternating")]
    sets.append(([(1 << 10, 9), (1 << 7, 7), (1 << 7, 64), (1 << 3, 17), (1, 8)], "mixed"))
    mm = p3.MerkleTreeMmcs(hash=hash_name)
    assert p3.get_thread_profile() == "latency"
    try:
        for dims, what in sets:
            if what == "mixed":
                mats = [_tree_matrix(("all P-1", "alternating", "all 0")[k % 3], h, w) for k, (h, w) in enumerate(dims)]
            else:
                mats = [_tree_matrix(what, *dims[0])]
            with _threads(oracle):
                oroot, otree = oracle.mmcs_commit(mats, kind)
            olayers = otree.layers()
            maxh = max(h for h, _ in dims)
            for profile in ("throughput", "latency"):
                p3.set_thread_profile(profile)
                root, tree = mm.commit(mats)
                tag = (hash_name, profile, dims, what)
                assert np.array_equal(root, oroot), tag
                glayers = tree.digest_layers()
                assert len(glayers) == len(olayers), tag
                for gl, ol in zip(glayers, olayers):
                    assert np.array_equal(gl, ol), tag + (len(ol),)
                for idx in sorted({0, maxh - 1, int(rng.integers(0, maxh))}):
                    rows, path = mm.open_batch(idx, tree)
                    orows, opath = otree.open_batch(idx)
                    assert np.array_equal(np.concatenate(rows), orows) and np.array_equal(path, opath), tag + (idx,)
                    assert oracle.mmcs_verify_batch(root, dims, idx, np.concatenate(rows), path, kind=kind), tag + (idx,)
                tree.free()
    finally:
        p3.set_thread_profile("latency")


@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
def test_hiding_tree_over_an_all_p_minus_1_matrix(p3, oracle, hash_name):
    """MerkleTreeHidingMmcs: the salts come from the MMCS's own stream, so this is the salted-leaf path with extreme words next
    to random ones (leaves m || salt); root, layers and openings against the oracle tree over the same interleaved list."""
    kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
    mmcs = p3.MerkleTreeHidingMmcs(hash_name, seed=1)
    host = oracle.rng_seed_from_u64(1)
    for dims in ([(1 << 9, 6)], [(1 << 6, 2), (1 << 6, 17), (8, 3)]):
        mats = [np.full(d, P - 1, dtype=np.uint32) for d in dims]
        root, tree = mmcs.commit(mats)
        inter = []
        for m in mats:
            inter += [m, oracle.rng_fill_field(host, m.shape[0] * 4).reshape(m.shape[0], 4)]
        exp_root, otree = oracle.mmcs_commit(inter, kind=kind)
        assert np.array_equal(root, exp_root), (hash_name, dims)
        for gl, ol in zip(tree.digest_layers(), otree.layers()):
            assert np.array_equal(gl, ol), (hash_name, dims, len(ol))
        idims = [(m.shape[0], m.shape[1]) for m in inter]
        for index in (0, 5, dims[0][0] - 1):
            vals, (salts, path) = mmcs.open_batch(index, tree)
            orows, opath = otree.open_batch(index)
            got = np.concatenate([np.concatenate([v, s]) for v, s in zip(vals, salts)])
            assert np.array_equal(got, orows) and np.array_equal(path, opath), (hash_name, dims, index)
            assert all((v == P - 1).all() for v in vals)
            assert oracle.mmcs_verify_batch(root, idims, index, got, path, kind=kind)
        tree.free()


# ---------------------------------------------------------------- E. proofs of degenerate instances
DEGENERATE = [(0, 0), (P, 2 * P), (2 ** 64 - 1, 2 ** 64 - 1), (P - 1, P - 1), (P - 1, 1)]
LOG_NS = [1, 3, 6, 10, 14, 16, 17]  # one-launch hiding sizes, FRI-tail-only sizes, and 16 / 17: the trace LDE on the fp64 narrow plan
T = (1, 0, 10, 4)
COMBOS = [(h, hid, pf) for h in ("poseidon2", "keccak") for hid in (False, True) for pf in ("latency", "throughput")]


@functools.lru_cache(maxsize=None)
def _oracle_proof(a, b, log_n, hash_name, hiding, t=T):
    from oracle import oracle as o
    kind = o.HASH_KECCAK if hash_name == "keccak" else o.HASH_POSEIDON2
    o.set_threads(o.test_threads())
    try:
        if hiding:
            return o.prove_fib_air_hiding(a, b, log_n, o.FriParams(*t), hash=kind, seed=1)
        return o.prove_fib_air(a, b, log_n, o.FriParams(*t), hash=kind)
    finally:
        o.set_threads(1)


def _same(proof, ref, what):
    assert len(proof) == len(ref), (what, len(proof), len(ref))
    if proof != ref:
        w1, w2 = np.frombuffer(proof, np.uint32), np.frombuffer(ref, np.uint32)
        pytest.fail("%s: proof words differ first at %d of %d" % (what, int(np.nonzero(w1 != w2)[0][0]), len(w1)))


def _prove_and_compare(p3, oracle, a, b, log_n, hash_name, hiding, profile):
    kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
    what = ("(%d, %d)" % (a, b), log_n, hash_name, "hiding" if hiding else "plain", profile)
    pr = p3.FibAirProver(log_n, params=p3.FriParameters(*T), hash=hash_name, hiding=hiding, seed=1, profile=profile)
    try:
        proof = pr.prove(a, b)
    finally:
        pr.close()
    _same(proof, _oracle_proof(a, b, log_n, hash_name, hiding), what)
    x = oracle.fib_public_x(a, b, 1 << log_n)
    overify = oracle.verify_fib_air_hiding if hiding else oracle.verify_fib_air
    assert overify(proof, a, b, x, log_n, oracle.FriParams(*T), hash=kind) == 0, what


@pytest.mark.parametrize("log_n", LOG_NS)
def test_all_zero_instance_every_configuration(p3, oracle, log_n):
    """prove(0, 0): a zero trace, a zero quotient, zero FRI layers and a zero final polynomial — both hashes, plain and hiding,
    both profiles: the complete proof bytes are the oracle prover's and the oracle verifier accepts."""
    for hash_name, hiding, profile in COMBOS:
        _prove_and_compare(p3, oracle, 0, 0, log_n, hash_name, hiding, profile)


@pytest.mark.parametrize("k,ab", list(enumerate(DEGENERATE))[1:])
def test_unreduced_and_extreme_instances(p3, oracle, k, ab):
    """a, b >= P up to 2^64 - 1 (legal at the C ABI; the trace generator reduces them, the public values take a path of their own)
    and the extreme reduced pairs, at every size; hash, hiding and profile in turn so that each pair meets each of them."""
    for i, log_n in enumerate(LOG_NS):
        for hash_name, hiding, profile in (COMBOS[(3 * k + i) % 8], COMBOS[(3 * k + i + 5) % 8]):
            _prove_and_compare(p3, oracle, ab[0], ab[1], log_n, hash_name, hiding, profile)
    assert _oracle_proof(P, 2 * P, 3, "poseidon2", False) == _oracle_proof(0, 0, 3, "poseidon2", False)


def test_all_zero_instance_at_the_headline_size(p3, oracle):
    """(0, 0) at 2^20 rows, plain, Poseidon2, the benchmark's FRI parameters (100 queries, 16 proof-of-work bits)."""
    t = (1, 0, 100, 16)
    pr = p3.FibAirProver(20, params=p3.FriParameters(*t))
    try:
        proof = pr.prove(0, 0)
        _same(proof, _oracle_proof(0, 0, 20, "poseidon2", False, t), "(0, 0) at 2^20")
        assert oracle.verify_fib_air(proof, 0, 0, 0, 20, oracle.FriParams(*t)) == 0
        assert pr.prove(P, 2 * P) == proof
    finally:
        pr.close()


def _dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("hash_name", ["poseidon2", "keccak"])
@pytest.mark.parametrize("log_n", [3, 10, 16])
def test_prove_trace_on_zero_constant_and_alternating_traces(p3, oracle, log_n, hash_name, hiding):
    """prove_trace: the all-zero trace with public values (0, 0, 0) gives the bytes of prove(0, 0) and check_fib_trace finds no
    bad row in it; a constant-P-1 trace and an alternating (P-1, 0) trace are committed as given (the trace commitment is the
    oracle's commitment of that matrix's LDE), proven, and rejected by both verifiers."""
    n = 1 << log_n
    kind = oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2
    gfp, ofp = p3.FriParameters(*T), oracle.FriParams(*T)
    overify = oracle.verify_fib_air_hiding if hiding else oracle.verify_fib_air
    pr = p3.FibAirProver(log_n, params=gfp, hash=hash_name, hiding=hiding, seed=1)
    try:
        zero = np.zeros((n, 2), dtype=np.uint32)
        assert p3.check_fib_trace(_dev(zero), [0, 0, 0]) == (None, 0, 0)
        ref = pr.prove(0, 0)
        _same(pr.prove_trace(_dev(zero), [0, 0, 0]), ref, "zero trace, device entry")
        _same(pr.prove_trace(zero, [0, 0, 0], check=True), ref, "zero trace, host entry, checked")
        _same(ref, _oracle_proof(0, 0, log_n, hash_name, hiding), "prove(0, 0) vs oracle")
        alt = si.alternating(log_n, P - 1, 0)
        for what, trace in (("const P-1", np.full((n, 2), P - 1, dtype=np.uint32)), ("alternating", np.stack([alt, alt], axis=1))):
            pis = [P - 1, 5, 7]
            bad_row, mask, count = p3.check_fib_trace(_dev(trace), pis)
            assert bad_row == 0 and mask and count >= n - 1, what
            proof = pr.prove_trace(_dev(trace), pis)
            assert proof and pr.prove_trace(trace, pis) == proof, what
            if not hiding:
                with _threads(oracle):
                    root, _ = oracle.mmcs_commit([oracle.coset_lde_batch(trace, gfp.log_blowup, p3.GENERATOR_MONTY, True)], kind)
                assert np.array_equal(np.frombuffer(proof[12:44], np.uint32), root), what
            with pytest.raises(p3.P3HipError):
                p3.verify_fib_air(proof, *pis, log_n, params=gfp, hash=hash_name, hiding=hiding)
            assert overify(proof, *pis, log_n, ofp, hash=kind) != 0, what
        assert pr.prove(0, 0) == ref
    finally:
        pr.close()


@pytest.mark.parametrize("hiding", [False, True])
def test_pool_batch_mixing_zero_and_ordinary_instances(p3, oracle, hiding):
    """One batch through the pool's scatter / gather with (0, 0) and its unreduced twin between ordinary instances: every
    instance comes back with its own bytes."""
    log_n = 10
    inst = [(3, 5), (0, 0), (7, 11), (P, 2 * P), (0, 0), (P - 1, 1), (0, 1), (2 ** 64 - 1, 2 ** 64 - 1), (0, 0)]
    pool = p3.FibAirBatchProver(log_n, n_provers=4, params=p3.FriParameters(*T), hiding=hiding)
    try:
        proofs = pool.prove(inst)
    finally:
        pool.close()
    for (a, b), pf in zip(inst, proofs):
        _same(pf, _oracle_proof(a, b, log_n, "poseidon2", hiding), "pool instance (%d, %d)" % (a, b))
    assert proofs[1] == proofs[3] == proofs[4] and proofs[0] != proofs[1]
