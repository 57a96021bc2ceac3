"""The BUFFER CONTRACT of the C ABI's device entries (include/p3hip.h; the table in DESIGN.md "Test strategy"): alignment, extent written,
read-only inputs, aliasing.

Every other GPU test reaches the kernels through the Python wrappers, whose buffers are fresh torch allocations: 512-byte aligned, of
exactly the output's size, rounded up by the allocator.  Here the test owns every buffer (tests/dev_buffers.py): inputs and outputs sit
INSIDE one allocation each, 0..3 words past a 512-byte boundary, with 0xDEADBEEF sentinel words all round.  Every result is compared
with the oracle bit for bit (never with the same entry on aligned buffers), and every case asserts that the guards on both sides of
every output are intact and that every input is unchanged.  The only "bad" pointers are those an entry refuses on the host before any
launch."""
import ctypes as C
import functools

import numpy as np
import pytest

import dev_buffers as db

pytestmark = pytest.mark.gpu

P = 0x78000001
BAD_ARG = -1
# (input words, output words) past a 512-byte boundary: 0 and 2 keep 8-byte alignment, 1 and 3 do not; only 0 keeps 16 bytes
OFFSET_PAIRS = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (3, 1), (2, 3)]


def _L(p3):
    return p3._lib.lib()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    import torch
    torch.cuda.synchronize()


def _vp(g):
    return C.c_void_p(g if isinstance(g, int) else g.data_ptr())


def _ok(p3, rc):
    assert rc == 0, (rc, p3._lib.take_last_error())


def _refused(p3, rc, text):
    msg = p3._lib.take_last_error() or ""
    assert rc == BAD_ARG and text in msg, (rc, msg)


def _field(seed, *shape):
    return np.random.default_rng(seed).integers(0, P, shape, dtype=np.uint64).astype(np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------
# transforms
# ------------------------------------------------------------------------------------------------
# One shape per plan the dispatcher (csrc/ntt.hip split_digits / launch_pass / lde_fused / lde_narrow) can pick, the smallest that
# reaches it.  Tiles hold up to 2^9 points: heights up to 2^9 are one pass, 2^10 .. 2^18 two, from 2^19 three.
#   2^0 x 2  a copy            2^3 x 3, 2^9 x 2  one pass (the 9-stage digit is the general kernel)
#   2^10 x 2, 2^12 x 4  two passes, fast kernels (power-of-two width)      2^13 x 5  two passes, general kernels (odd width)
#   2^15 x 2, 2^16 x 2  two passes below / at the height where the narrow LDE plan starts      2^17 x 3  digits (8, 9) swapped
#   2^19 x 1  three passes
GENERAL = [(0, 2), (3, 3), (9, 2), (10, 2), (12, 4), (13, 5), (15, 2), (16, 2), (17, 3), (19, 1)]
# coset LDE at blowup 2, bit-reversed out (what the provers and the PCS run), besides the shapes above:
#   2^18 x 1  the fused middle (three forward digits; width 1 is outside the narrow plan)
#   2^16 x 2 / 4 / 6  the narrow three-launch plan: it runs at offsets 0 and 2, and at offsets 1 and 3 the 8-byte check of lde_narrow
#             sends the same shape to the general plans
#   2^21 x 2  the smallest height at which all three narrow kernels use 8-byte lane vectors
#   2^16 x 64 / 65  the wide two-digit plan: single words per lane (Vec<1> in csrc/ntt_narrow.hip.h), so it takes any 4-byte alignment
LDE_EXTRA = [(18, 1), (16, 4), (16, 6), (21, 2), (16, 64), (16, 65)]
ADDED = 1

OPS = {
    "dft": GENERAL, "idft": GENERAL, "coset_dft": GENERAL, "bit_reverse_rows": GENERAL,
    "coset_lde_natural": GENERAL + [(16, 4)], "coset_lde_bitrev": GENERAL + LDE_EXTRA, "coset_lde_from_coeffs": GENERAL + LDE_EXTRA,
}
TRANSFORM_CASES = [(op, lh, w) for op, shapes in OPS.items() for lh, w in shapes]


def _out_rows(op, h):
    return h << ADDED if op.startswith("coset_lde") else h


@functools.lru_cache(maxsize=None)
def _transform_ref(op, log_h, w):
    """(input, expected) of one transform, computed once by the oracle and shared read-only"""
    from oracle import oracle as o
    import __graft_entry__ as ge
    shift = ge.load_package().GENERATOR_MONTY
    h = 1 << log_h
    x = _field(1000 * log_h + w, h, w)
    o.set_threads(o.test_threads() if log_h >= 21 else 1)
    try:
        if op == "dft":
            y = o.dft_batch(x)
        elif op == "idft":
            y = o.idft_batch(x)
        elif op == "coset_dft":
            y = o.coset_dft_batch(x, shift)
        elif op == "bit_reverse_rows":
            y = o.bit_reverse_rows(x)
        elif op == "coset_lde_natural":
            y = o.coset_lde_batch(x, ADDED, shift, False)
        elif op == "coset_lde_bitrev":
            y = o.coset_lde_batch(x, ADDED, shift, True)
        else:  # coefficients in: coset_dft_batch of the zero-padded matrix, then bit_reverse_rows (include/p3hip.h)
            y = o.bit_reverse_rows(o.coset_dft_batch(np.concatenate([x, np.zeros(((h << ADDED) - h, w), np.uint32)]), shift))
    finally:
        o.set_threads(1)
    return _frozen(x, np.ascontiguousarray(y))


def _run_transform(p3, op, d_in, d_out, h, w):
    L, st, shift = _L(p3), _stream(), p3.GENERATOR_MONTY
    if op == "dft":
        return L.p3hip_dft_batch_bb31_dev(d_in, d_out, h, w, st)
    if op == "idft":
        return L.p3hip_idft_batch_bb31_dev(d_in, d_out, h, w, st)
    if op == "coset_dft":
        return L.p3hip_coset_dft_batch_bb31_dev(d_in, d_out, h, w, shift, st)
    if op == "bit_reverse_rows":
        return L.p3hip_bit_reverse_rows_dev(d_in, d_out, h, w, st)
    if op == "coset_lde_natural":
        return L.p3hip_coset_lde_batch_bb31_dev(d_in, d_out, h, w, ADDED, shift, 0, st)
    if op == "coset_lde_bitrev":
        return L.p3hip_coset_lde_batch_bb31_dev(d_in, d_out, h, w, ADDED, shift, 1, st)
    return L.p3hip_coset_lde_from_coeffs_bb31_dev(d_in, d_out, h, w, ADDED, shift, st)


@pytest.mark.parametrize("op,log_h,w", TRANSFORM_CASES, ids=["%s-2^%dx%d" % c for c in TRANSFORM_CASES])
def test_transform_at_offsets(p3, oracle, op, log_h, w):
    h = 1 << log_h
    x, want = _transform_ref(op, log_h, w)
    for off_in, off_out in OFFSET_PAIRS:
        what = "%s 2^%d x %d, input +%d words, output +%d words" % (op, log_h, w, off_in, off_out)
        src = db.place(x, off_in)
        dst = db.guarded(want.size, off_out)
        _ok(p3, _run_transform(p3, op, _vp(src), _vp(dst), h, w))
        _sync()
        got = dst.host().reshape(want.shape)
        assert np.array_equal(got, want), "%s: first differing word %d" % (what, int(np.nonzero(got.reshape(-1) != want.reshape(-1))[0][0]))
        dst.assert_guards_intact(what + ": d_out")
        src.assert_unchanged(what + ": d_in")


IN_PLACE = [(lh, w) for lh, w in GENERAL if lh <= 16]


@pytest.mark.parametrize("op", ["dft", "idft"])
@pytest.mark.parametrize("log_h,w", IN_PLACE, ids=["2^%dx%d" % s for s in IN_PLACE])
def test_dft_in_place_then_out_of_place(p3, oracle, op, log_h, w):
    """d_out == d_in is supported by dft and idft: the input is staged in scratch slot 0 of the stream.  An out-of-place call on the
    same stream straight after must still be right: it queues behind the in-place one, whose scratch it may reuse."""
    h = 1 << log_h
    x, want = _transform_ref(op, log_h, w)
    other_shape = (12, 4) if (log_h, w) != (12, 4) else (10, 2)
    x2, want2 = _transform_ref(op, *other_shape)
    for off in (0, 1, 2, 3):
        buf = db.place(x, off)
        src2, dst2 = db.place(x2, 3 - off), db.guarded(want2.size, off)
        _ok(p3, _run_transform(p3, op, _vp(buf), _vp(buf), h, w))
        _ok(p3, _run_transform(p3, op, _vp(src2), _vp(dst2), 1 << other_shape[0], other_shape[1]))
        _sync()
        assert np.array_equal(buf.host().reshape(want.shape), want), (op, log_h, w, off)
        buf.assert_guards_intact("in-place buffer")
        assert np.array_equal(dst2.host().reshape(want2.shape), want2), (op, other_shape, off, "after the in-place call")
        dst2.assert_guards_intact("d_out of the call after")
        src2.assert_unchanged("d_in of the call after")


REFUSING = ["coset_dft", "coset_lde_natural", "coset_lde_bitrev", "coset_lde_from_coeffs", "bit_reverse_rows"]


@pytest.mark.parametrize("op", REFUSING + ["dft", "idft"])
def test_overlapping_ranges_are_refused(p3, oracle, op):
    """Two ranges that overlap without being identical are refused by every transform entry, identical ones by all but dft / idft,
    before anything is launched: P3HIP_ERR_BAD_ARG, and every word of the allocation stays as it was."""
    log_h, w = 3, 3
    h, out_words = 1 << log_h, _out_rows(op, 1 << log_h) * w
    x = _field(7, h, w)
    # one allocation holding input and output: the view is large enough for every placement below
    span = 2 * out_words + h * w
    cases = [("d_out = d_in + 1 row", out_words, out_words + w),          # (input word, output word) inside the view
             ("d_out ending inside d_in", out_words, out_words + w - out_words),
             ("d_out = d_in + 1 word", out_words, out_words + 1)]
    if op in REFUSING:
        cases.append(("d_out == d_in", out_words, out_words))
    for what, i_in, i_out in cases:
        assert 0 <= i_out and i_out + out_words <= span and i_in + h * w <= span
        buf = db.guarded(span, 1)
        buf.view[i_in:i_in + h * w].copy_(__import__("torch").from_numpy(x.reshape(-1).view(np.int32)))
        before = buf.host()
        base = buf.data_ptr()
        rc = _run_transform(p3, op, _vp(base + 4 * i_in), _vp(base + 4 * i_out), h, w)
        _sync()
        _refused(p3, rc, "overlap" if i_in != i_out else "")
        assert np.array_equal(buf.host(), before), (op, what, "a refused call wrote")
        buf.assert_guards_intact(what)


# ------------------------------------------------------------------------------------------------
# generators: the SmallRng stream and the Fibonacci trace
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_rng_fill_at_offsets(p3, oracle, n):
    """Word-wise stores: any 4-byte alignment.  Exactly n words are written; the stream and the generator state afterwards are the
    host stream's (the state of an unguarded fill of the same n is pinned against the same host state by tests/test_gpu_hiding.py)."""
    L = _L(p3)
    for off in (0, 1, 2, 3):
        host = oracle.rng_seed_from_u64(5)
        want = oracle.rng_fill_field(host, n)
        h = C.c_void_p()
        _ok(p3, L.p3hip_rng_create(5, C.byref(h)))
        try:
            out = db.guarded(n, off)
            _ok(p3, L.p3hip_rng_fill_field_dev(h, _vp(out), n, _stream()))
            state = (C.c_uint64 * 4)()
            _ok(p3, L.p3hip_rng_state(h, state, _stream()))
            assert np.array_equal(out.host(), want), (n, off)
            out.assert_guards_intact("rng fill n = %d at +%d words" % (n, off))
            assert list(state) == list(host), (n, off)
            # an unguarded fill of the same n leaves the same state
            h2 = C.c_void_p()
            _ok(p3, L.p3hip_rng_create(5, C.byref(h2)))
            plain = __import__("torch").empty(n, dtype=__import__("torch").int32, device="cuda")
            _ok(p3, L.p3hip_rng_fill_field_dev(h2, _vp(plain), n, _stream()))
            state2 = (C.c_uint64 * 4)()
            _ok(p3, L.p3hip_rng_state(h2, state2, _stream()))
            L.p3hip_rng_destroy(h2)
            assert list(state2) == list(state)
        finally:
            L.p3hip_rng_destroy(h)


@pytest.mark.parametrize("n", [1, 2, 8, 1024])
def test_fib_trace_at_offsets(p3, oracle, n):
    """Rows are stored as 8-byte pairs: d_out is 8-byte aligned by contract (offsets 0 and 2 run), anything else is refused."""
    L = _L(p3)
    want = oracle.generate_trace_rows(3, 5, n)
    for off in (0, 1, 2, 3):
        out = db.guarded(2 * n, off)
        rc = L.p3hip_fib_trace_dev(3, 5, n, _vp(out), _stream())
        _sync()
        if off % 2:
            _refused(p3, rc, "fib_trace: d_out must be 8-byte aligned")
            assert (out.host() == db.SENTINEL).all()
        else:
            _ok(p3, rc)
            assert np.array_equal(out.host().reshape(n, 2), want), (n, off)
        out.assert_guards_intact("fib trace n = %d at +%d words" % (n, off))


# ------------------------------------------------------------------------------------------------
# hash primitives
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _poseidon2_ref(n):
    from oracle import oracle as o
    x = _field(40 + n, n, 16)
    return _frozen(x, np.stack([o.poseidon2_permute(s) for s in x]))


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_poseidon2_permute_at_offsets(p3, oracle, n):
    """The production entry takes any 4-byte alignment: 16-byte-aligned states run the fp64 per-lane form (16-byte pieces), every
    other alignment falls back to the 16-lane form, which moves single words.  The diagnostic entry refuses what its form cannot take."""
    L = _L(p3)
    x, want = _poseidon2_ref(n)
    for off in (0, 1, 2, 3, 4):
        buf = db.guarded(16 * n, off).fill(x)
        _ok(p3, L.p3hip_poseidon2_permute_dev(_vp(buf), n, _stream()))
        _sync()
        assert np.array_equal(buf.host().reshape(n, 16), want), (n, off)
        buf.assert_guards_intact("poseidon2 states at +%d words" % off)
    for variant in (0, 1, 2, 3):
        for off in (1, 2):
            buf = db.guarded(16 * n, off).fill(x)
            rc = L.p3hip_poseidon2_permute_variant_dev(_vp(buf), n, variant, _stream())
            _sync()
            if variant == 3:
                _ok(p3, rc)
                assert np.array_equal(buf.host().reshape(n, 16), want), (n, off)
            else:
                _refused(p3, rc, "d_states must be 16-byte aligned")
                assert np.array_equal(buf.host().reshape(n, 16), x)
            buf.assert_guards_intact()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_keccak_f_at_offsets(p3, oracle, n):
    """[u64; 25] states: 8-byte aligned by contract (word offsets 0 and 2 run; 8-byte loads and stores only), 4-byte offsets are
    refused by both entries."""
    L = _L(p3)
    x = np.random.default_rng(50 + n).integers(0, 1 << 63, (n, 25), dtype=np.uint64) * 2 + 1
    want = np.stack([oracle.keccak_f(s) for s in x])
    for off in (0, 1, 2, 3):
        buf = db.guarded(50 * n, off).fill(x.view(np.uint32))
        rc = L.p3hip_keccak_f_dev(_vp(buf), n, _stream())
        _sync()
        if off % 2:
            _refused(p3, rc, "keccak_f: d_states must be 8-byte aligned")
            assert np.array_equal(buf.host(), x.view(np.uint32).reshape(-1))
            _refused(p3, L.p3hip_keccak_f_variant_dev(_vp(buf), n, 0, _stream()), "d_states must be 8-byte aligned")
        else:
            _ok(p3, rc)
            assert np.array_equal(buf.host().view(np.uint64).reshape(n, 25), want), (n, off)
        buf.assert_guards_intact("keccak states at +%d words" % off)


# ------------------------------------------------------------------------------------------------
# MMCS
# ------------------------------------------------------------------------------------------------
# One case per leaf kernel mmcs_commit can choose, at the smallest height that reaches it: (hash, profile, [(log_h, w)], what)
MMCS_CASES = [
    ("poseidon2", "latency", [(5, 3)], "leaf_coop: one dense matrix below 2^12 rows"),
    ("poseidon2", "latency", [(12, 5)], "leaf_hash_q4: 2^12 rows, w <= 64, latency profile"),
    ("poseidon2", "throughput", [(12, 5)], "leaf_hash_f64: the same under the throughput profile"),
    ("poseidon2", "throughput", [(12, 64)], "leaf_hash_f64_wide: w = 64"),
    ("poseidon2", "latency", [(12, 70)], "leaf_hash_f64_wide: w = 70 (above the quad form's 64)"),
    ("poseidon2", "latency", [(12, 3), (12, 2)], "leaf_hash_f64_rowset: two matrices at 2^12 rows"),
    ("poseidon2", "latency", [(5, 3), (5, 2)], "leaf_hash: two matrices at 2^5 rows"),
    ("poseidon2", "latency", [(6, 3), (4, 5)], "mixed heights: 2^4 rows injected into a compress layer"),
    ("keccak", "latency", [(5, 68)], "keccak_leaf_wide: w = 68"),
    ("keccak", "latency", [(5, 3)], "keccak_leaf: the generic kernel"),
    ("keccak", "latency", [(6, 3), (4, 5)], "keccak mixed heights"),
]


def _mats_at(case_mats, off, seed):
    return [db.place(_field(seed + i, 1 << lh, w), (off + i) % 4) for i, (lh, w) in enumerate(case_mats)]


def _tree_args(mats, shapes):
    n = len(mats)
    return ((C.c_void_p * n)(*[m.data_ptr() for m in mats]), (C.c_size_t * n)(*[1 << lh for lh, _ in shapes]),
            (C.c_size_t * n)(*[w for _, w in shapes]), n)


def _layers_of(p3, tree):
    """every digest layer of a tree, downloaded"""
    import torch
    L = _L(p3)
    out = []
    for l in range(L.p3hip_mmcs_num_layers(tree)):
        ln = C.c_size_t()
        ptr = L.p3hip_mmcs_layer_dev(tree, l, C.byref(ln))
        host = np.zeros((ln.value, 8), np.uint32)
        _ok(p3, L.p3hip_download(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), host.nbytes))
        out.append(host)
    return out


@pytest.mark.parametrize("hash,profile,shapes,what", MMCS_CASES, ids=[c[3].split(":")[0] + "-" + c[1] for c in MMCS_CASES])
def test_mmcs_commit_at_offsets(p3, oracle, hash, profile, shapes, what):
    """commit_dev (Poseidon2) / commit_hash_dev with the matrices at word offsets 0..3, and commit_into_dev into a guarded buffer of
    exactly p3hip_mmcs_layer_words words: root and every layer equal the oracle's, the matrices are unchanged."""
    L = _L(p3)
    kind = oracle.HASH_KECCAK if hash == "keccak" else oracle.HASH_POSEIDON2
    p3.set_thread_profile(profile)
    try:
        for off in (0, 1, 2, 3):
            mats = _mats_at(shapes, off, 60)
            want_root, otree = oracle.mmcs_commit([m._expected.reshape(1 << lh, w) for m, (lh, w) in zip(mats, shapes)], kind=kind)
            want_layers = otree.layers()
            ptrs, hs, ws, n = _tree_args(mats, shapes)
            for entry in ("commit", "commit_into"):
                root, tree = np.zeros(8, np.uint32), C.c_void_p()
                if entry == "commit" and kind == oracle.HASH_POSEIDON2:
                    _ok(p3, L.p3hip_mmcs_commit_dev(ptrs, hs, ws, n, root.ctypes.data_as(C.c_void_p), C.byref(tree), _stream()))
                elif entry == "commit":
                    _ok(p3, L.p3hip_mmcs_commit_hash_dev(kind, ptrs, hs, ws, n, root.ctypes.data_as(C.c_void_p), C.byref(tree), _stream()))
                else:
                    words = L.p3hip_mmcs_layer_words(max(1 << lh for lh, _ in shapes))
                    assert words == 8 * sum(len(l) for l in want_layers)
                    store = db.guarded(words, 0)
                    _ok(p3, L.p3hip_mmcs_commit_into_dev(kind, ptrs, hs, ws, n, _vp(store), C.byref(tree), _stream()))
                    _ok(p3, L.p3hip_mmcs_root(tree, root.ctypes.data_as(C.c_void_p), _stream()))
                try:
                    _sync()
                    assert np.array_equal(root, want_root), (what, entry, off)
                    got_layers = _layers_of(p3, tree)
                    assert len(got_layers) == len(want_layers)
                    for l, (g, w_) in enumerate(zip(got_layers, want_layers)):
                        assert np.array_equal(g, w_), (what, entry, off, "layer", l)
                    if entry == "commit_into":
                        assert np.array_equal(store.host(), np.concatenate([l.reshape(-1) for l in want_layers]))
                        store.assert_guards_intact(what + ": d_layers")
                finally:
                    L.p3hip_mmcs_free(tree)
            for m in mats:
                m.assert_unchanged(what + ": matrix at +%d words" % m.offset)
    finally:
        p3.set_thread_profile("latency")


@pytest.mark.parametrize("hash", ["poseidon2", "keccak"])
def test_mmcs_commit_into_refuses_misaligned_layers(p3, oracle, hash):
    """Digests move as 16-byte pieces in every compression kernel: d_layers is 16-byte aligned by contract.  8-byte and 4-byte
    offsets are refused on the host; nothing is written."""
    L = _L(p3)
    kind = oracle.HASH_KECCAK if hash == "keccak" else oracle.HASH_POSEIDON2
    shapes = [(5, 3)]
    mats = _mats_at(shapes, 0, 61)
    ptrs, hs, ws, n = _tree_args(mats, shapes)
    words = L.p3hip_mmcs_layer_words(32)
    for off in (2, 1, 3):
        store, tree = db.guarded(words, off), C.c_void_p()
        rc = L.p3hip_mmcs_commit_into_dev(kind, ptrs, hs, ws, n, _vp(store), C.byref(tree), _stream())
        _sync()
        _refused(p3, rc, "mmcs_commit_into: d_layers must be 16-byte aligned")
        assert not tree.value and (store.host() == db.SENTINEL).all()
        store.assert_guards_intact()


@pytest.mark.parametrize("hash", ["poseidon2", "keccak"])
@pytest.mark.parametrize("w", [4, 6, 8])
def test_hiding_mmcs_commit_at_offsets(p3, oracle, hash, w):
    """MerkleTreeHidingMmcs: the salted Keccak leaf kernel takes 16-byte rows (8-byte for width 6) and the commit falls back to the
    generic kernel otherwise (csrc/mmcs.hip launch_keccak_leaf_salted): both sides of that check, and Poseidon2's rowset kernel, equal
    the oracle tree over the interleaved (matrix, salt) list."""
    L = _L(p3)
    kind = oracle.HASH_KECCAK if hash == "keccak" else oracle.HASH_POSEIDON2
    log_h = 6
    for off in (0, 1, 2, 3):
        mat = db.place(_field(70 + w, 1 << log_h, w), off)
        host = oracle.rng_seed_from_u64(3)
        salt = oracle.rng_fill_field(host, 4 << log_h).reshape(1 << log_h, 4)
        want_root, otree = oracle.mmcs_commit([mat._expected.reshape(1 << log_h, w), salt], kind=kind)
        rng, tree, root = C.c_void_p(), C.c_void_p(), np.zeros(8, np.uint32)
        _ok(p3, L.p3hip_rng_create(3, C.byref(rng)))
        ptrs, hs, ws, n = _tree_args([mat], [(log_h, w)])
        try:
            _ok(p3, L.p3hip_mmcs_commit_hiding_dev(kind, ptrs, hs, ws, n, rng, root.ctypes.data_as(C.c_void_p), C.byref(tree), _stream()))
            _sync()
            assert np.array_equal(root, want_root), (hash, w, off)
            for l, (g, w_) in enumerate(zip(_layers_of(p3, tree), otree.layers())):
                assert np.array_equal(g, w_), (hash, w, off, "layer", l)
        finally:
            if tree.value:
                L.p3hip_mmcs_free(tree)
            L.p3hip_rng_destroy(rng)
        mat.assert_unchanged("matrix of the hiding commit")


@pytest.mark.parametrize("hash", ["poseidon2", "keccak"])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_mmcs_open_and_verify_many_at_offsets(p3, oracle, hash, n):
    """open_batch_many_dev writes exactly n x row_words and n x depth x 8 words; verify_batch_many_dev writes exactly n status words
    and one counter.  d_indices and d_rows at word offsets 1..3 (word-wise accesses), d_paths 16-byte aligned by contract."""
    L = _L(p3)
    kind = oracle.HASH_KECCAK if hash == "keccak" else oracle.HASH_POSEIDON2
    shapes = [(6, 3), (4, 5)]
    depth, rw = 6, 8
    mats = _mats_at(shapes, 1, 80)
    host_mats = [m._expected.reshape(1 << lh, w) for m, (lh, w) in zip(mats, shapes)]
    want_root, otree = oracle.mmcs_commit(host_mats, kind=kind)
    ptrs, hs, ws, nm = _tree_args(mats, shapes)
    root, tree = np.zeros(8, np.uint32), C.c_void_p()
    _ok(p3, L.p3hip_mmcs_commit_hash_dev(kind, ptrs, hs, ws, nm, root.ctypes.data_as(C.c_void_p), C.byref(tree), _stream()))
    try:
        assert L.p3hip_mmcs_row_words(tree) == rw
        idx = np.random.default_rng(n).integers(0, 1 << depth, n, dtype=np.uint64).astype(np.uint32)
        want_rows = np.zeros((n, rw), np.uint32)
        want_paths = np.zeros((n, depth, 8), np.uint32)
        for i, ix in enumerate(idx):
            want_rows[i], want_paths[i] = otree.open_batch(int(ix))
        for off in (1, 2, 3):
            d_idx = db.place(idx, off)
            d_rows, d_paths = db.guarded(n * rw, (off + 1) % 4 or 1), db.guarded(n * depth * 8, 0)
            _ok(p3, L.p3hip_mmcs_open_batch_many_dev(tree, _vp(d_idx), n, _vp(d_rows), _vp(d_paths), _stream()))
            _sync()
            assert np.array_equal(d_rows.host().reshape(n, rw), want_rows), (n, off)
            assert np.array_equal(d_paths.host().reshape(n, depth, 8), want_paths), (n, off)
            d_rows.assert_guards_intact("d_rows")
            d_paths.assert_guards_intact("d_paths")
            # verify what was opened, with one opening tampered: exactly n status words and the counter
            rows_in = want_rows.copy()
            rows_in[n // 2, 0] ^= 1
            rows_in[n // 2, 0] %= P
            d_rows_in = db.place(rows_in, off)
            d_paths_in = db.place(want_paths, 0)
            status, rejected = db.guarded(n, off), db.guarded(1, off)
            _ok(p3, L.p3hip_mmcs_verify_batch_many_dev(kind, root.ctypes.data_as(C.c_void_p), hs, ws, nm, _vp(d_idx), n, _vp(d_rows_in),
                                                       _vp(d_paths_in), _vp(status), _vp(rejected), _stream()))
            _sync()
            want_status = np.zeros(n, np.uint32)
            want_status[n // 2] = 1  # P3HIP_MMCS_ROOT_MISMATCH, as the oracle's verify_batch says
            assert not oracle.mmcs_verify_batch(want_root, [(64, 3), (16, 5)], int(idx[n // 2]), rows_in[n // 2], want_paths[n // 2], kind=kind)
            assert np.array_equal(status.host(), want_status), (n, off)
            assert rejected.host()[0] == 1
            status.assert_guards_intact("d_status")
            rejected.assert_guards_intact("d_rejected")
            for g, name in ((d_idx, "d_indices"), (d_rows_in, "d_rows"), (d_paths_in, "d_paths")):
                g.assert_unchanged(name)
            # a d_paths that is not 16-byte aligned is refused
            for bad in (1, 2):
                d_paths_bad = db.place(want_paths, bad)
                status2 = db.guarded(n, 0)
                rc = L.p3hip_mmcs_verify_batch_many_dev(kind, root.ctypes.data_as(C.c_void_p), hs, ws, nm, _vp(d_idx), n, _vp(d_rows_in),
                                                        _vp(d_paths_bad), _vp(status2), None, _stream())
                _sync()
                _refused(p3, rc, "d_paths must be 16-byte aligned")
                assert (status2.host() == db.SENTINEL).all()
        for m in mats:
            m.assert_unchanged("matrix")
    finally:
        L.p3hip_mmcs_free(tree)


# ------------------------------------------------------------------------------------------------
# provers: a caller's trace, read in place
# ------------------------------------------------------------------------------------------------
GFP = (1, 0, 10, 4)
PROVE_CASES = [(h, hid, ln) for h in ("poseidon2", "keccak") for hid in (False, True) for ln in (3, 10)] + [("poseidon2", False, 16), ("keccak", False, 16)]


@functools.lru_cache(maxsize=None)
def _fib_ref(hash, hiding, log_n, a=7, b=11):
    from oracle import oracle as o
    kind = o.HASH_KECCAK if hash == "keccak" else o.HASH_POSEIDON2
    fp = o.FriParams(*GFP)
    proof = o.prove_fib_air_hiding(a, b, log_n, fp, hash=kind, seed=1) if hiding else o.prove_fib_air(a, b, log_n, fp, hash=kind)
    trace = o.generate_trace_rows(a, b, 1 << log_n)
    trace.setflags(write=False)
    return trace, [a, b, o.fib_public_x(a, b, 1 << log_n)], proof


@pytest.mark.parametrize("hash,hiding,log_n", PROVE_CASES)
def test_prove_trace_dev_at_offsets(p3, oracle, hash, hiding, log_n):
    """d_trace inside a larger allocation at word offsets 0..3.  The hiding prover reads rows as 8-byte pairs with no fallback
    (randomize_trace_kernel), so the contract of the three trace entries is 8-byte aligned, as p3hip_fib_check_trace_dev's: offsets 0
    and 2 give the oracle's bytes and leave the trace unchanged, offsets 1 and 3 are refused before anything is launched.  At 2^16 rows
    the trace LDE is the narrow plan's."""
    n = 1 << log_n
    trace, pis, want = _fib_ref(hash, hiding, log_n)
    pr = p3.FibAirProver(log_n, params=p3.FriParameters(*GFP), hash=hash, hiding=hiding)
    try:
        for off in (0, 1, 2, 3):
            buf = db.place(trace, off)
            t = buf.view.view(n, 2)
            if off % 2:
                with pytest.raises(p3.P3HipError, match="fib_prover_prove_trace_dev: the trace must be 8-byte aligned"):
                    pr.prove_trace(t, pis)
                if not hiding:
                    with pytest.raises(p3.P3HipError, match="fib_prover_enqueue_trace_dev: the trace must be 8-byte aligned"):
                        pr.enqueue_trace(t, pis)
            else:
                assert pr.prove_trace(t, pis) == want, (hash, hiding, log_n, off)
                if not hiding:
                    pr.enqueue_trace(t, pis)
                    assert pr.finish() == want, (hash, hiding, log_n, off, "enqueue / finish")
            buf.assert_unchanged("d_trace at +%d words" % off)
    finally:
        pr.close()


@pytest.mark.parametrize("hiding", [False, True])
def test_batch_prove_traces_dev_at_offsets(p3, oracle, hiding):
    log_n = 10
    n = 1 << log_n
    trace, pis, want = _fib_ref("poseidon2", hiding, log_n)
    pool = p3.FibAirBatchProver(log_n, n_provers=2, params=p3.FriParameters(*GFP), hiding=hiding)
    try:
        bufs = [db.place(trace, off) for off in (0, 2, 2, 0)]
        assert pool.prove_traces([b.view.view(n, 2) for b in bufs], [pis] * 4) == [want] * 4
        odd = db.place(trace, 3)
        with pytest.raises(p3.P3HipError, match="the trace must be 8-byte aligned"):
            pool.prove_traces([bufs[0].view.view(n, 2), odd.view.view(n, 2)], [pis] * 2)
        for b in bufs + [odd]:
            b.assert_unchanged("d_traces[i]")
    finally:
        pool.close()


@pytest.mark.parametrize("hash,hiding", [("poseidon2", False), ("keccak", True)])
def test_prove_into_writes_exactly_the_proof(p3, oracle, hash, hiding):
    """The host `out` of p3hip_fib_prover_prove_into: cap == len exactly fills it and nothing else; cap == len - 1 is refused and
    nothing is written, before and after the prover knows its proofs' length."""
    log_n, guard = 5, 64
    _, _, want = _fib_ref(hash, hiding, log_n)
    ln = len(want)
    for first_cap in (ln - 1, ln):  # a fresh prover learns the length from its first proof
        pr = p3.FibAirProver(log_n, params=p3.FriParameters(*GFP), hash=hash, hiding=hiding)
        try:
            for cap in (first_cap, ln - 1, ln):
                host = np.full(ln + 2 * guard, 0xEF, dtype=np.uint8)
                if cap < ln:
                    with pytest.raises(p3.P3HipError, match="the proof needs %d bytes" % ln):
                        pr.prove_into(7, 11, host.ctypes.data + guard, cap)
                    assert (host == 0xEF).all(), "a refused prove_into wrote"
                else:
                    assert pr.prove_into(7, 11, host.ctypes.data + guard, cap) == ln
                    assert host[guard:guard + ln].tobytes() == want
                    assert (host[:guard] == 0xEF).all() and (host[guard + ln:] == 0xEF).all()
        finally:
            pr.close()


# ------------------------------------------------------------------------------------------------
# PCS: evaluations read in place at any 4-byte alignment
# ------------------------------------------------------------------------------------------------
PCS_T = (1, 0, 3, 2)
PREFIX = np.arange(1, 6, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _pcs_ref(flavour, kind, log_h):
    """(rounds, roots, opened, proof, the next transcript sample) of the reference provers of tests/pcs_ref.py, pcs_hiding_ref.py and
    pcs_mixed_ref.py; rounds = [[(evals, shift or None, [points])]]"""
    import pcs_hiding_ref as H
    import pcs_mixed_ref as MR
    import pcs_ref as R
    rng = np.random.default_rng(900 + 10 * log_h + kind)
    w = 3 if log_h == 4 else 2
    z0, z1 = R.rand_point(rng), R.rand_point(rng)
    ch = R.RefChallenger(kind)
    ch.observe(PREFIX)
    if flavour == "mixed":
        rounds = [[(R.rand_matrix(rng, 10, 2), None, [z0]), (R.rand_matrix(rng, 4, 3), R.rand_shift(rng), [z1, z0])]]
        d = MR.prove(kind, PCS_T, rounds, ch)
        roots, opened, proof = d["roots"], d["opened"], d["proof"]
    elif flavour == "hiding":
        rounds = [[(R.rand_matrix(rng, log_h, w), R.rand_shift(rng), [z0, z1])]]
        ref = H.HidingPcs(kind, PCS_T, 4, 1, 1)
        com = ref.commit([(m, s) for m, s, _ in rounds[0]])
        opened, proof = ref.open([(com, [pts for _, _, pts in rounds[0]])], ch)
        roots = [com.root]
    else:
        rounds = [[(R.rand_matrix(rng, log_h, w), R.rand_shift(rng), [z0, z1])]]
        opened, proof, roots = R.open_with_roots(kind, PCS_T, log_h, rounds, ch)
    return rounds, roots, opened, proof, ch.sample_ext()


PCS_CASES = [(f, h, lh) for f in ("plain", "hiding") for h in (("poseidon2", 0), ("keccak", 1)) for lh in (4, 10)] + [("mixed", ("poseidon2", 0), 10)]


@pytest.mark.parametrize("flavour,hk,log_h", PCS_CASES, ids=["%s-%s-2^%d" % (f, h[0], lh) for f, h, lh in PCS_CASES])
def test_pcs_commit_and_open_at_offsets(p3, oracle, flavour, hk, log_h):
    """p3hip_pcs_commit_dev reads d_evals in place: through the LDE plans (word-wise, or the narrow plan behind its check) on a plain
    object, word by word in the randomizing kernel of a hiding one.  Roots, opened values, proof bytes and the transcript afterwards
    equal the reference prover's at every offset, and the evaluations are unchanged after commit and open."""
    hash, kind = hk
    rounds, roots, opened, proof, nxt = _pcs_ref(flavour, kind, log_h)
    for off in (0, 1, 2, 3):
        if flavour == "hiding":
            pcs = p3.HidingFriPcs(p3.FriParameters(*PCS_T), hash)
        else:
            pcs = p3.TwoAdicFriPcs(p3.FriParameters(*PCS_T), hash, mixed_heights=flavour == "mixed")
        try:
            bufs, datas = [], []
            for r, mats in enumerate(rounds):
                these = [db.place(m, (off + i) % 4) for i, (m, _, _) in enumerate(mats)]
                bufs += these
                root, data = pcs.commit([(b.view.view(*m.shape), s) for b, (m, s, _) in zip(these, mats)])
                assert np.array_equal(root, roots[r]), (flavour, hash, log_h, off, "root of round", r)
                datas.append(data)
            for b in bufs:
                b.assert_unchanged("d_evals after commit")
            ch = p3.Challenger(hash)
            ch.observe(PREFIX)
            got_opened, got_proof = pcs.open([(d, [pts for _, _, pts in mats]) for d, mats in zip(datas, rounds)], ch)
            assert np.array_equal(got_opened, opened), (flavour, hash, log_h, off)
            assert got_proof == proof, (flavour, hash, log_h, off)
            assert np.array_equal(ch.sample_ext(), nxt)
            for b in bufs:
                b.assert_unchanged("d_evals after open")
            for d in datas:
                d.free()
        finally:
            pcs.free()


# ------------------------------------------------------------------------------------------------
# caller-defined AIRs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib", "B"])
def test_air_quotient_and_check_trace_at_offsets(p3, oracle, name):
    """d_lde and d_trace at any 4-byte alignment (word-wise loads); every chunk is a 16-byte-aligned buffer of exactly n x 4 words
    (one 16-byte store per row): guarded, and a chunk pointer that is 8-byte but not 16-byte aligned is refused."""
    import air_ref as A
    import pcs_ref as R
    air, gen = A.all_airs(p3)[name]
    log_n, lqd = 4, air.log_quotient_degree
    n = 1 << log_n
    rng = np.random.default_rng(31)
    trace = R.rand_matrix(rng, log_n, air.width)
    pis, alpha = R.O.to_monty(rng.integers(0, P, air.n_public, dtype=np.uint64)), R.rand_point(rng)
    lde = oracle.coset_lde_batch(trace, lqd + 1, p3.GENERATOR_MONTY, True)
    want = A.quotient_chunks(air.code, air.consts, lde[:n << lqd], log_n, pis, alpha)
    L = _L(p3)
    pp, al = np.ascontiguousarray(pis, np.uint32), np.ascontiguousarray(alpha, np.uint32)

    def run(d_lde, chunks):
        ptrs = (C.c_void_p * air.n_chunks)(*[c.data_ptr() for c in chunks])
        return L.p3hip_air_quotient_dev(air._h, _stream(), _vp(d_lde), log_n, lqd + 1, pp.ctypes.data_as(C.c_void_p), al.ctypes.data_as(C.c_void_p), ptrs)

    for off in (0, 1, 2, 3):
        d_lde = db.place(lde, off)
        chunks = [db.guarded(4 * n, 0) for _ in range(air.n_chunks)]
        _ok(p3, run(d_lde, chunks))
        _sync()
        for c, (g, w_) in enumerate(zip(chunks, want)):
            assert np.array_equal(g.host().reshape(n, 4), w_), (name, off, c)
            g.assert_guards_intact("chunk %d" % c)
        d_lde.assert_unchanged("d_lde at +%d words" % off)
    # the last chunk 8-byte but not 16-byte aligned: refused, nothing written
    d_lde = db.place(lde, 0)
    chunks = [db.guarded(4 * n, 0) for _ in range(air.n_chunks - 1)] + [db.guarded(4 * n, 2)]
    rc = run(d_lde, chunks)
    _sync()
    _refused(p3, rc, "chunk %d must be a 16-byte aligned device pointer" % (air.n_chunks - 1))
    for g in chunks:
        assert (g.host() == db.SENTINEL).all()
        g.assert_guards_intact()
    # check_trace: a valid trace and one with a broken row, at offsets 1..3
    good, gpis = gen(log_n)
    bad = good.copy()
    bad[5, 0] = (int(bad[5, 0]) + 1) % P
    for tr in (good, bad):
        want_ct = A.check_trace(air.code, air.consts, tr, gpis)
        for off in (1, 2, 3):
            d_tr = db.place(tr, off)
            assert air.check_trace(d_tr.view.view(n, air.width), gpis) == want_ct, (name, off)
            d_tr.assert_unchanged("d_trace at +%d words" % off)


# ------------------------------------------------------------------------------------------------
# device verifiers: exactly n status words
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,hiding", [("poseidon2", False), ("keccak", True)])
def test_fib_verifier_dev_writes_exactly_n_statuses(p3, oracle, hash, hiding):
    """n = 3 proofs on a verifier created for 8: d_status is a guarded buffer of exactly 3 words, d_rejected one guarded word; d_proofs
    sits at a 4-byte offset with the stride at the proof length rounded up to 4.  One accepted member, one with a tampered proof word,
    one with another public value: the statuses are the host verifier's."""
    log_n = 5
    kind = oracle.HASH_KECCAK if hash == "keccak" else oracle.HASH_POSEIDON2
    trace, pis, proof = _fib_ref(hash, hiding, log_n)
    a, b, x = pis
    words = np.frombuffer(proof, np.uint32).copy()
    words[-3] = (int(words[-3]) + 1) % P  # a coefficient of the final polynomial (the witness is the last word), still canonical
    members = [(proof, x), (words.tobytes(), x), (proof, (x + 1) % P)]
    L, gfp = _L(p3), p3.FriParameters(*GFP)._c()
    verify = L.p3hip_verify_fib_air_hiding if hiding else L.p3hip_verify_fib_air_hash
    host = [verify(kind, (C.c_uint8 * len(pf)).from_buffer_copy(pf), len(pf), a, b, xx, log_n, C.cast(gfp, C.c_void_p)) for pf, xx in members]
    p3._lib.take_last_error()
    assert host[0] == 0 and all(h in (10, 11, 13, 14, 15) for h in host[1:]), host  # codes the device reports as they are
    v = p3.FibAirVerifier(log_n, p3.FriParameters(*GFP), hash, hiding, max_proofs=8)
    try:
        stride = (v.proof_len + 3) // 4 * 4
        assert stride == len(proof)
        for off in (1, 2, 3):
            d_proofs = db.place(np.concatenate([np.frombuffer(pf, np.uint32) for pf, _ in members]), off)
            d_pis = db.place(np.stack([oracle.to_monty(np.array([a, b, xx], dtype=np.uint64)) for _, xx in members]), off)
            status, rejected = db.guarded(3, off), db.guarded(1, (off + 1) % 4)
            v.verify_many_dev(d_proofs.view, d_pis.view.view(3, 3), n=3, stride=stride, status=status.view, rejected=rejected.view)
            _sync()
            assert list(status.host()) == host, (hash, hiding, off)
            assert rejected.host()[0] == 2
            status.assert_guards_intact("d_status")
            rejected.assert_guards_intact("d_rejected")
            d_proofs.assert_unchanged("d_proofs")
            d_pis.assert_unchanged("d_pis")
    finally:
        v.close()


@pytest.mark.parametrize("hash,hiding", [("poseidon2", False), ("keccak", True)])
def test_pcs_verifier_dev_writes_exactly_n_statuses(p3, oracle, hash, hiding):
    """The same for p3hip_pcs_verifier_verify_dev: d_status (3 words), d_rejected and d_chal_out (3 x 128 words, 8-byte aligned by
    contract) guarded; proofs, roots, points and opened values at 4-byte offsets; the transcripts in at an 8-byte one.  (The alignment
    refusals of this entry are pinned by tests/test_gpu_pcs_verify_many.py::test_batch_mechanics.)"""
    import pcs_many as M
    from test_gpu_pcs_verify_many import Case, same_transcript
    case = Case(p3, hash, hiding, 3, (1, 0, 3, 2), [[2, 5], [3]], [[[0, 1], [0]], [[1]]], 3, 8100 + int(hiding))
    members = [dict(m) for m in case.members]
    for j in (1, 2):
        t = np.frombuffer(members[j]["proof"], dtype=np.uint32).copy()
        free = np.nonzero(case.classes != M.SHAPE)[0]
        i = int(free[(37 * j) % len(free)])
        t[i] = M.tampered(t[i])
        members[j]["proof"] = t.tobytes()
    want = [case.expected(m)[0] for m in members]
    assert want[0] == 0 and want[1] and want[2], want
    v = case.verifier(8)
    sw = p3.pcs.STATE_WORDS
    try:
        assert v.proof_len % 4 == 0
        stack = lambda k: np.stack([m[k] for m in members])
        for off in (1, 2, 3):
            ins = dict(proofs=db.place(np.concatenate([np.frombuffer(m["proof"], np.uint32) for m in members]), off),
                       roots=db.place(stack("roots"), off), points=db.place(stack("points"), (off + 1) % 4),
                       opened=db.place(stack("opened"), (off + 2) % 4), state=db.place(stack("state"), 2))
            status, rejected, chal_out = db.guarded(3, off), db.guarded(1, off), db.guarded(3 * sw, 2)
            v.verify_many_dev(ins["proofs"].view, ins["roots"].view, ins["points"].view, ins["opened"].view, ins["state"].view.view(3, sw), n=3,
                              stride=v.proof_len, status=status.view, rejected=rejected.view, chal_out=chal_out.view)
            _sync()
            assert list(status.host()) == want, (hash, hiding, off)
            assert rejected.host()[0] == 2
            for g, name in ((status, "d_status"), (rejected, "d_rejected"), (chal_out, "d_chal_out")):
                g.assert_guards_intact(name)
            after = p3.Challenger(hash)
            after.import_state(chal_out.host()[:sw])
            assert same_transcript(after, members[0]["after"].clone())
            for name, g in ins.items():
                g.assert_unchanged("d_" + name)
    finally:
        v.close()


def test_probe_entries_refuse_misaligned_doubles(p3, oracle):
    """The diagnostic probes read and write doubles: their buffers are 8-byte aligned by contract, and a 4-byte offset is refused on the
    host.  The word ops of the field probe take any 4-byte alignment."""
    L = _L(p3)
    n = 5
    d_in, d_out = db.guarded(2 * 16 * n, 1), db.guarded(16 * n, 1)
    _refused(p3, L.p3hip_poseidon2_f64_probe_dev(_vp(d_in), _vp(d_out), n, 0, _stream()), "probe: d_in holds doubles and must be 8-byte aligned")
    for off_in, off_out in ((1, 0), (0, 1)):
        a, b = db.guarded(2 * 2 * n, off_in), db.guarded(2 * n, off_out)
        _refused(p3, L.p3hip_field_probe_dev(32, _vp(a), _vp(b), n, _stream()), "must be 8-byte aligned")
        _sync()
        assert (b.host() == db.SENTINEL).all()
    x = _field(5, n, 2)
    for off in (1, 2, 3):
        a, b = db.place(x, off), db.guarded(n, 4 - off)
        _ok(p3, L.p3hip_field_probe_dev(1, _vp(a), _vp(b), n, _stream()))  # add
        _sync()
        assert np.array_equal(b.host(), (x[:, 0].astype(np.uint64) + x[:, 1]) % P)
        b.assert_guards_intact("d_out of the word probe")
        a.assert_unchanged("d_in of the word probe")
    _sync()
    assert (d_out.host() == db.SENTINEL).all()


@pytest.mark.parametrize("hash,kind", [("poseidon2", 0), ("keccak", 1)])
def test_pcs_commit_quotient_at_offsets(p3, oracle, hash, kind):
    """p3hip_pcs_commit_quotient_dev reads d_chunks[c] through the inverse transform into the object's own buffer (word-wise; the 16-byte
    pieces of the blinding kernel touch owned memory only): any 4-byte alignment, read-only.  The root equals the reference prover's."""
    import pcs_hiding_ref as H
    import pcs_ref as R
    rng = np.random.default_rng(77 + kind)
    log_h, wq = 4, 4  # wq a multiple of four: the blinding kernel's 16-byte form
    for n_chunks in (2, 4):
        chunks = [R.rand_matrix(rng, log_h, wq) for _ in range(n_chunks)]
        want = H.HidingPcs(kind, PCS_T, 4, 1, 1).commit_quotient(chunks).root
        for off in (0, 1, 2, 3):
            pcs = p3.HidingFriPcs(p3.FriParameters(*PCS_T), hash)
            try:
                bufs = [db.place(c, (off + i) % 4) for i, c in enumerate(chunks)]
                root, data = pcs.commit_quotient([b.view.view(1 << log_h, wq) for b in bufs])
                assert np.array_equal(root, want), (hash, n_chunks, off)
                for b in bufs:
                    b.assert_unchanged("d_chunks[c] at +%d words" % b.offset)
                data.free()
            finally:
                pcs.free()
