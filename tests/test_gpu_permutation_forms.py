"""Every formulation of the two permutations, state by state, on the GPU.

Poseidon2 has four (p2::permute: int32, one state per lane; p2f::permute: exact integers in fp64, one per lane; p2q::permute: fp64,
one per DPP quad; p2c::permute: int32, one per 16-lane row), Keccak-f three (kk::permute; kk::permute_digest: peeled first round, last
round computes row 0 only; kk::f_coop: one state per wave).  Which one hashes a given Merkle layer depends on the layer's length and
the thread profile, and through trees and proofs each sees only pseudo-random digests at a few power-of-two sizes.  Here each runs
alone (p3hip_poseidon2_permute_variant_dev, p3hip_keccak_f_variant_dev), and the production compression kernels run once each on a
caller's layer (p3hip_compress_layer_variant_dev), on
  - the pre-image families of tests/poseidon2_sched_ref.py: canonical states whose S-box outputs at a chosen round are +-(P - 1)/2
    patterns, so that the fp64 forms run at the largest magnitudes words in [0, P) can produce (the internal rounds entered at
    35 (P + 1)/2 in all sixteen elements; x15 lanes at 2^50.66 before a fold);
  - every single-bit Keccak state and its complement, so that a wrong rotation count, lane mapping or bank mask is located by the
    failing case itself;
  - state counts that leave a quad, a 16-lane row, a wave and a workgroup partly filled.
Every comparison is array_equal.  Nothing here aims at a fault: every launch is in bounds for any input words."""
import ctypes as C

import numpy as np
import pytest

import field_ref as F
import poseidon2_sched_ref as S
import pyref

pytestmark = pytest.mark.gpu
P, H = F.P, S.H
P2_VARIANTS = (0, 1, 2, 3)
P2_NAMES = {0: "p2 (int32, per lane)", 1: "p2f (fp64, per lane)", 2: "p2q (fp64, per quad)", 3: "p2c (int32, per 16 lanes)"}
GUARD = 0xdeadbeef
_cache = {}


def _permute(p3, words, variant, guard=2):
    """the chosen form on (n, 16) Montgomery words; `guard` states of sentinel words before and after the buffer must stay untouched"""
    import torch
    n = len(words)
    buf = np.full((n + 2 * guard, 16), GUARD, dtype=np.uint32)
    buf[guard:guard + n] = words
    d = p3.dev_u32(buf)
    p3.mmcs.poseidon2_permute_variant(d[guard:guard + n], variant)
    torch.cuda.synchronize()
    out = p3.host_u32(d)
    assert np.all(out[:guard] == GUARD) and np.all(out[guard + n:] == GUARD), "variant %d wrote outside its %d states" % (variant, n)
    return out[guard:guard + n]


def _random_states():
    if "rand" not in _cache:
        rng = np.random.default_rng([F.SEED, 32])
        st = rng.integers(0, P, size=(1 << 16, 16), dtype=np.uint32)
        for i, e in enumerate(S.EDGE_STATES):
            st[i] = F.v_monty(np.array(e, np.uint64))
        st.setflags(write=False)
        _cache["rand"] = st
    return _cache["rand"]


@pytest.fixture(scope="module")
def random_expected(oracle):
    """the oracle's permutation of the 2^16 random states, computed once"""
    st = _random_states()
    exp = np.stack([oracle.poseidon2_permute(s) for s in st])
    exp.setflags(write=False)
    return exp


def _family_words():
    """(Montgomery words of every family state, Montgomery words of pyref.poseidon2 of it), rolled so that row 0 is 'all +h' at seam 3"""
    if "fam" not in _cache:
        n = len(S.targets())
        st = np.roll(F.v_monty(S.family_states()).astype(np.uint32), -3 * n, axis=0)
        exp = np.roll(F.v_monty(S.family_expected()).astype(np.uint32), -3 * n, axis=0)
        fam = S.family()[3 * n:] + S.family()[:3 * n]
        assert fam[0][:2] == ("all +h", 3) and fam[1][:2] == ("all -h", 3)
        st.setflags(write=False)
        exp.setflags(write=False)
        _cache["fam"] = (st, exp, fam)
    return _cache["fam"]


def _first_bad(got, want):
    bad = np.flatnonzero(np.any(got != want, axis=1))
    return None if bad.size == 0 else (int(bad.size), int(bad[0]))


# ---- Poseidon2: the four forms on whole states ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", P2_VARIANTS)
def test_poseidon2_random_states(p3, random_expected, variant):
    """2^16 seeded random states (the four edge states first) against the oracle's permutation: all four forms give the same words."""
    got = _permute(p3, _random_states(), variant)
    bad = _first_bad(got, random_expected)
    assert bad is None, "%s: %d states differ, first %d: got %r want %r" % (
        P2_NAMES[variant], bad[0], bad[1], got[bad[1]].tolist(), random_expected[bad[1]].tolist())


def test_poseidon2_public_entries_agree(p3, random_expected):
    """poseidon2_permute, through the host entry and the device entry, on the same 2^16 states"""
    import torch
    st = _random_states()
    assert np.array_equal(p3.poseidon2_permute(st), random_expected)
    d = p3.dev_u32(np.array(st))
    p3.poseidon2_permute(d)
    torch.cuda.synchronize()
    assert np.array_equal(p3.host_u32(d), random_expected)


def _assert_family_is_adversarial():
    """Asserted first by the family tests, so that they cannot quietly stop being adversarial: rows 0 and 1 of the family are the
    all-+-h targets at seam 3, the canonical states of words in [0, P) on which BOTH exact schedule models enter the internal rounds
    at +-35 (P - 1)/2 or -+35 (P + 1)/2 (the S-box's other representative; which, is its rounding) in all sixteen elements."""
    st, _, fam = _family_words()
    if _cache.get("adversarial"):
        return
    for row, sign in ((0, 1), (1, -1)):
        state = [int(v) for v in F.v_canon(st[row])]
        assert tuple(state) == fam[row][3] and fam[row][2] == (sign * H,) * 16 and all(0 <= v < P for v in state)
        for model in (S.model_f, S.model_q):
            entry = model(state)[1]
            assert len(set(entry)) == 1 and entry[0] in (sign * 35.0 * H, -sign * 35.0 * (H + 1)), entry[:2]
    _cache["adversarial"] = True


@pytest.mark.parametrize("variant", P2_VARIANTS)
def test_poseidon2_families(p3, variant):
    """Every family state (each target at every seam) against pyref.poseidon2; the seam-7 states also against their closed form, one
    external linear layer of the chosen S-box outputs, which needs no reference."""
    _assert_family_is_adversarial()
    st, exp, fam = _family_words()
    got = _permute(p3, st, variant)
    bad = _first_bad(got, exp)
    assert bad is None, "%s: %d family states differ, first: %r at seam %d: got %r want %r" % (
        P2_NAMES[variant], bad[0], fam[bad[1]][0], fam[bad[1]][1], F.v_canon(got[bad[1]]).tolist(), F.v_canon(exp[bad[1]]).tolist())
    seen = 0
    for i, (name, seam, y, _) in enumerate(fam):
        if seam == 7:
            assert F.v_canon(got[i]).tolist() == S.seam7_closed_form(y), (P2_NAMES[variant], name)
            seen += 1
    assert seen == len(S.targets())
    assert F.v_canon(got[[f[:2] for f in fam].index(("all +h", 7))]).tolist() == [35 * H % P] * 16


# one wave, one workgroup and one workgroup + 1 of each launch geometry (states per wave: 64, 16, 4), and the whole family; the
# levels kernel of variant 3 takes powers of two only: one row, one wave, one workgroup (16 out of a chunk of 32), two, and 1024
P2_LAYER_SIZES = {0: (64, 256, 257, 824), 1: (64, 256, 257, 824), 2: (16, 64, 65, 824), 3: (1, 4, 16, 32, 1024)}


@pytest.mark.parametrize("variant", P2_VARIANTS)
def test_poseidon2_compression_layer_on_the_families(p3, variant):
    """The PRODUCTION compression kernel of each form (compress_layer_kernel without injection, compress_layer_f64_kernel,
    compress_layer_q4_kernel, one level of tree_levels_coop_kernel), launched once on a layer whose child-digest pairs are the family
    states: the digest is the first eight words of the permutation.  compress_layer_q4_kernel itself then runs at its worst case."""
    import torch
    _assert_family_is_adversarial()
    st, exp, fam = _family_words()
    assert len(st) == 824
    for n_out in P2_LAYER_SIZES[variant]:
        idx = np.arange(n_out) % len(st)
        layer = p3.dev_u32(np.ascontiguousarray(st[idx].reshape(2 * n_out, 8)))
        out = p3.mmcs.compress_layer_variant("poseidon2", variant, layer)
        torch.cuda.synchronize()
        got = p3.host_u32(out)
        bad = _first_bad(got, exp[idx][:, :8])
        assert bad is None, "%s, n_out = %d: %d digests differ, first %d (%r at seam %d)" % (
            P2_NAMES[variant], n_out, bad[0], bad[1], fam[idx[bad[1]]][0], fam[idx[bad[1]]][1])
        assert np.array_equal(p3.host_u32(layer).reshape(n_out, 16), st[idx])  # the caller's layer is read only


@pytest.mark.parametrize("variant", (2, 3))
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257))
def test_poseidon2_state_counts(p3, random_expected, variant, n):
    """A partly filled quad, 16-lane row, wave and workgroup: the idle lanes run the permutation on zeros and write nothing.  Each
    result is compared whole, and the words just before and after the n states stay untouched."""
    st = _random_states()[100:100 + n]
    assert np.array_equal(_permute(p3, st, variant), random_expected[100:100 + n])
    fam_st, fam_exp, _ = _family_words()
    assert np.array_equal(_permute(p3, fam_st[:n], variant), fam_exp[:n])


def _probe(p3, states_f64, mode):
    import torch
    from plonky3_mobile_amd import _lib
    d = torch.from_numpy(np.ascontiguousarray(states_f64, dtype=np.float64)).cuda()
    out = torch.empty(d.shape, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().p3hip_poseidon2_f64_probe_dev(C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), d.shape[0], mode,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def test_quad_form_on_doubles(p3):
    """Mode 3 of the fp64 probe: p2q::permute on integer-valued doubles — the canonical edges, their negatives, the rounding-tie
    neighbourhoods of reduce, +-2^33 in all sixteen elements and in alternation, and 200 random states up to +-2^33 — against
    big-integer arithmetic, and against mode 0 (p2f::permute on the same doubles).  The count is no multiple of 16: the last wave
    holds idle quads."""
    B = 2 ** 33
    rng = np.random.default_rng([F.SEED, 33])
    states = [[v] * 16 for v in (0, 1, -1, P - 1, 1 - P, P, -P, P // 2, P // 2 + 1, -(P // 2), -(P // 2 + 1), B, -B, B - 1, 1 - B)]
    states += [[B * (1, -1)[i & 1] for i in range(16)], [B * (-1, 1)[i & 1] for i in range(16)], [B * s for s in S.V_SIGN],
               [B if i in S.INTEGER_LANES else 0 for i in range(16)], [-B if i in S.INTEGER_LANES else 0 for i in range(16)],
               [(B - i) * (1, -1)[i >> 1 & 1] for i in range(16)]]
    for k in (0, 1, 2, 3):  # the half-way points of the quotient estimate below 2^33, as in the reduce test
        states.append([((2 * k + 1) * P + (-3, -1, 1, 3)[i & 3]) // 2 * (1, -1)[i >> 2 & 1] for i in range(16)])
    states += [[int(v) for v in row] for row in rng.integers(-B, B + 1, size=(200, 16))]
    assert len(states) % 16 and all(abs(v) <= B for row in states for v in row)
    arr = np.array(states, dtype=np.float64)
    assert all(int(a) == b for a, b in zip(arr.reshape(-1), [v for row in states for v in row]))
    want = np.array([pyref.poseidon2([v % P for v in row]) for row in states], dtype=np.uint64)
    got = F.v_canon(_probe(p3, arr, 3))
    bad = _first_bad(got, want)
    assert bad is None, "p2q on doubles: %d states differ, first %d: in %r" % (bad[0], bad[1], states[bad[1]])
    assert np.array_equal(F.v_canon(_probe(p3, arr, 0)), want)


# ---- Keccak-f ----------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
KECCAK_RC = (0x0000000000000001, 0x0000000000008082, 0x800000000000808a, 0x8000000080008000, 0x000000000000808b, 0x0000000080000001,
             0x8000000080008081, 0x8000000000008009, 0x000000000000008a, 0x0000000000000088, 0x0000000080008009, 0x000000008000000a,
             0x000000008000808b, 0x800000000000008b, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
             0x000000000000800a, 0x800000008000000a, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008)


def _rho_offsets():
    """FIPS 202, 3.2.2: the rotation of lane (x, y), from the walk (1, 0) -> (y, 2x + 3y) with offsets (t + 1)(t + 2) / 2"""
    r = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = (t + 1) * (t + 2) // 2 % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


def keccak_f_python(a):
    """Keccak-f[1600] on 25 Python integers, word x + 5y: FIPS 202 restated, sharing no table with the library or the C oracle except
    the round constants"""
    rot = lambda v, n: ((v << n) | (v >> (64 - n))) & M64 if n else v  # noqa: E731
    rho = _rho_offsets()
    a = list(a)
    for rc in KECCAK_RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rot(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rot(a[x + 5 * y], rho[x][y])
        a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & M64 & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
        a[0] ^= rc
    return a


def _keccak_states():
    """(states (n, 25) uint64, labels): the 1600 single-bit states, their complements, zero, ones, one word of ones, 4096 random"""
    if "kst" not in _cache:
        rows, labels = [], []
        for w in range(25):
            for z in range(64):
                s = np.zeros(25, np.uint64)
                s[w] = np.uint64(1 << z)
                rows.append(s)
                labels.append("bit (x=%d, y=%d, z=%d)" % (w % 5, w // 5, z))
        rows += [~r for r in rows[:1600]]
        labels += ["all but " + t for t in labels[:1600]]
        rows += [np.zeros(25, np.uint64), np.full(25, M64, np.uint64)]
        labels += ["zero", "ones"]
        for w in range(25):
            s = np.zeros(25, np.uint64)
            s[w] = np.uint64(M64)
            rows.append(s)
            labels.append("word (x=%d, y=%d) of ones" % (w % 5, w // 5))
        rng = np.random.default_rng([F.SEED, 34])
        rnd = rng.integers(0, 1 << 63, size=(4096, 25), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(4096, 25), dtype=np.uint64)
        rows += list(rnd)
        labels += ["random %d" % i for i in range(4096)]
        st = np.stack(rows)
        st.setflags(write=False)
        _cache["kst"] = (st, labels)
    return _cache["kst"]


@pytest.fixture(scope="module")
def keccak_expected(oracle):
    st, _ = _keccak_states()
    exp = np.stack([oracle.keccak_f(s) for s in st])
    exp.setflags(write=False)
    return exp


def test_keccak_reference_against_plain_python(keccak_expected):
    """the oracle's keccak_f on every single-bit state, on zero and on ones, against the pure-Python permutation above"""
    st, labels = _keccak_states()
    for i in list(range(1600)) + [3200, 3201]:
        assert keccak_expected[i].tolist() == keccak_f_python([int(v) for v in st[i]]), labels[i]


@pytest.mark.parametrize("variant", (0, 1, 2))
def test_keccak_f_forms(p3, keccak_expected, variant):
    """kk::permute, kk::permute_digest (words 0..3: the other words of the buffer stay as they were) and kk::f_coop (one state per wave:
    7323 waves) on the sparse, structured and random states.  A mismatch names the input and the first differing output word."""
    import torch
    st, labels = _keccak_states()
    guard = np.full((1, 25), 0x5a5a5a5a5a5a5a5a, np.uint64)
    d = torch.from_numpy(np.concatenate([guard, st, guard]).view(np.int64)).cuda()
    p3.mmcs.keccak_f_variant(d[1:1 + len(st)], variant)
    torch.cuda.synchronize()
    out = d.cpu().numpy().view(np.uint64)
    assert np.all(out[0] == guard) and np.all(out[-1] == guard)
    got, words = out[1:-1], (4 if variant == 1 else 25)
    bad = np.flatnonzero(np.any(got[:, :words] != keccak_expected[:, :words], axis=1))
    if bad.size:
        i = int(bad[0])
        w = int(np.flatnonzero(got[i, :words] != keccak_expected[i, :words])[0])
        pytest.fail("variant %d: %d of %d states differ; first: input %s, output word (x=%d, y=%d): got %016x want %016x; inputs: %r" % (
            variant, bad.size, len(st), labels[i], w % 5, w // 5, int(got[i, w]), int(keccak_expected[i, w]), [labels[j] for j in bad[:8]]))
    if variant == 1:
        assert np.array_equal(got[:, 4:], st[:, 4:])


@pytest.mark.parametrize("variant", (2,))
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5))
def test_keccak_coop_state_counts(p3, keccak_expected, variant, n):
    """one to five waves: a partly filled workgroup of the per-wave form"""
    import torch
    st, _ = _keccak_states()
    d = torch.from_numpy(np.array(st[3200 + 27:3200 + 27 + n]).view(np.int64)).cuda()
    p3.mmcs.keccak_f_variant(d, variant)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), keccak_expected[3200 + 27:3200 + 27 + n])


# one wave / workgroup / workgroup + 1 of the per-lane kernel; the levels kernels take powers of two: one compression, one chunk (128
# digests in per workgroup for the per-lane levels kernel, 16 for the per-wave one), several chunks
KECCAK_LAYER_SIZES = {0: (64, 256, 257, 1000), 1: (1, 2, 64, 128, 2048), 2: (1, 2, 8, 16, 1024)}


@pytest.mark.parametrize("variant", (0, 1, 2))
def test_keccak_compression_layer(p3, oracle, variant):
    """keccak_compress_kernel (no injection), keccak_tree_levels_kernel and keccak_tree_levels_coop_kernel (one level each) on random
    digest pairs and on pairs of all-ones and all-zero words, against the oracle's compression"""
    import torch
    if "klayer" not in _cache:
        rng = np.random.default_rng([F.SEED, 35])
        layer = rng.integers(0, 1 << 32, size=(4096, 8), dtype=np.uint32)
        ones, zero = np.full(8, 0xffffffff, np.uint32), np.zeros(8, np.uint32)
        layer[0], layer[1], layer[2], layer[3], layer[4], layer[5], layer[6], layer[7] = zero, zero, ones, ones, zero, ones, ones, zero
        layer[8] = [0xffffffff, 0] * 4
        layer[9] = [0, 0xffffffff] * 4
        exp = np.stack([oracle.keccak_compress(layer[2 * i], layer[2 * i + 1]) for i in range(2048)])
        _cache["klayer"] = (layer, exp)
    layer, exp = _cache["klayer"]
    for n_out in KECCAK_LAYER_SIZES[variant]:
        d = p3.dev_u32(np.ascontiguousarray(layer[:2 * n_out]))
        out = p3.mmcs.compress_layer_variant("keccak", variant, d)
        torch.cuda.synchronize()
        bad = _first_bad(p3.host_u32(out), exp[:n_out])
        assert bad is None, "Keccak form %d, n_out = %d: %d digests differ, first %d" % (variant, n_out, bad[0], bad[1])
        assert np.array_equal(p3.host_u32(d), layer[:2 * n_out])


def test_new_entries_refuse_bad_arguments(p3):
    """as test_device_probe_refuses_bad_arguments: unknown variants, modes and hashes, null pointers, a layer the levels kernels cannot
    take (never padded); n = 0 is a no-op; nothing is written by a refused call"""
    import torch
    from plonky3_mobile_amd import _lib
    lib = _lib.lib()
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    ptr = C.c_void_p(d.data_ptr())
    for v in (-1, 4):
        assert lib.p3hip_poseidon2_permute_variant_dev(ptr, 1, v, None) == -1 and "poseidon2 variant" in p3.take_last_error()
        assert lib.p3hip_poseidon2_f64_probe_dev(ptr, ptr, 1, v, None) == -1 and "probe mode" in p3.take_last_error()
    for v in (-1, 3):
        assert lib.p3hip_keccak_f_variant_dev(ptr, 1, v, None) == -1 and "keccak_f variant" in p3.take_last_error()
    for v in range(4):
        assert lib.p3hip_poseidon2_permute_variant_dev(None, 1, v, None) == -1 and "null" in p3.take_last_error()
        assert lib.p3hip_poseidon2_f64_probe_dev(None, ptr, 1, v, None) == -1 and "null" in p3.take_last_error()
        assert lib.p3hip_poseidon2_permute_variant_dev(ptr, 0, v, None) == 0 and lib.p3hip_poseidon2_f64_probe_dev(ptr, ptr, 0, v, None) == 0
    for v in range(3):
        assert lib.p3hip_keccak_f_variant_dev(None, 1, v, None) == -1 and "null" in p3.take_last_error()
        assert lib.p3hip_keccak_f_variant_dev(ptr, 0, v, None) == 0
    for hash, v in ((2, 0), (0, 4), (1, 3), (0, -1)):
        assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, ptr, 1, None) == -1 and "compress_layer_variant" in p3.take_last_error()
    for hash, v in ((0, 3), (1, 1), (1, 2)):
        assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, ptr, 3, None) == -1 and "power-of-two" in p3.take_last_error()
    for hash, v in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2)):
        assert lib.p3hip_compress_layer_variant_dev(hash, v, None, ptr, 1, None) == -1 and "null" in p3.take_last_error()
        assert lib.p3hip_compress_layer_variant_dev(hash, v, ptr, ptr, 0, None) == 0
    torch.cuda.synchronize()
    assert p3.take_last_error() is None and d.cpu().tolist() == [0.0] * 64
