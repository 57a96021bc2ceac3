"""mmcs_commit's driver logic — height classes, injection of shorter matrices, the host loops that fuse injection-free levels into one
launch, the leaf kernel chosen by shape, the caps — swept over the grid of tests/mmcs_classes.py.  Every comparison is np.array_equal
against oracle.mmcs_commit on the same matrices: the root and EVERY digest layer, under both thread profiles, for both hashes.  There is
no tolerance and no case is left out.  tests/test_mmcs_classes_host.py checks the same grid without a GPU: the oracle's trees against
an independent driver, and that the grid reaches every kernel and every `levels` value the commit can take."""
import zlib

import numpy as np
import pytest

import mmcs_classes as mc

pytestmark = pytest.mark.gpu
P = mc.P
ERR_BAD_ARG = -1  # P3HIP_ERR_BAD_ARG
N_MANY = 65


def _kind(oracle, hash_name):
    return oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2


def _commit(p3, mm, mats):
    """mm.commit(mats); where a matrix has no column, p3hip_mmcs_commit_hash_dev itself with a real one-word allocation in that
    matrix's place, so that no null pointer is involved (an empty torch tensor has none to give)"""
    if all(m.shape[1] for m in mats):
        return mm.commit(mats)
    import ctypes as C
    import torch
    dmats = [p3.dev_u32(m) for m in mats]
    spare = torch.zeros(1, dtype=torch.int32, device="cuda")
    n = len(dmats)
    ptrs = (C.c_void_p * n)(*[d.data_ptr() if d.numel() else spare.data_ptr() for d in dmats])
    assert all(ptrs)
    hs = (C.c_size_t * n)(*[d.shape[0] for d in dmats])
    ws = (C.c_size_t * n)(*[d.shape[1] for d in dmats])
    root, handle = np.zeros(8, dtype=np.uint32), C.c_void_p()
    p3._lib.check(p3._lib.lib().p3hip_mmcs_commit_hash_dev(mm._kind, ptrs, hs, ws, n, root.ctypes.data_as(C.c_void_p), C.byref(handle),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    tree = p3.MerkleTree(handle, dmats, root)
    tree.spare = spare  # lives as long as the tree that borrows it
    return root, tree


def _oracle_tree(oracle, mats, hash_name):
    """the reference: computed once per case, shared by both profiles, never written"""
    oracle.set_threads(oracle.test_threads())
    try:
        root, tree = oracle.mmcs_commit(mats, _kind(oracle, hash_name))
    finally:
        oracle.set_threads(1)
    layers = tree.layers()
    for l in layers:
        l.setflags(write=False)
    return root, tree, layers


def _same_tree(root, tree, oroot, olayers, tag):
    assert np.array_equal(root, oroot), tag
    got = tree.digest_layers()
    assert len(got) == len(olayers), tag
    for g, o in zip(got, olayers):
        assert np.array_equal(g, o), tag + (len(o),)


def _openings(p3, mm, tree, root, otree, dims, case_id, tag):
    """open_batch at 0, maxh - 1 and a seeded index; open_batch_many of 65 seeded indices, row for row; verify_batch_many accepts all
    of them, and rejects all of them with RootMismatch once one word of the last matrix's row is changed"""
    maxh = mc.tallest(dims)
    rng = np.random.default_rng([zlib.crc32(case_id.encode()), 7])
    for idx in sorted({0, maxh - 1, int(rng.integers(0, maxh))}):
        rows, path = mm.open_batch(idx, tree)
        orows, opath = otree.open_batch(idx)
        assert np.array_equal(np.concatenate(rows), orows) and np.array_equal(path, opath), tag + (idx,)
    indices = rng.integers(0, maxh, N_MANY).astype(np.uint32)
    rows, paths = mm.open_batch_many(indices, tree)
    grows, gpaths = p3.host_u32(rows), p3.host_u32(paths)
    for k, idx in enumerate(indices):
        orows, opath = otree.open_batch(int(idx))
        assert np.array_equal(grows[k], orows) and np.array_equal(gpaths[k], opath), tag + (k, int(idx))
    status = mm.verify_batch_many(root, dims, indices, rows, paths)
    assert not p3.host_u32(status).any(), tag
    if rows.shape[1]:  # a commitment of zero-width matrices alone opens no word
        bad = rows.clone()
        bad[:, -1] = (bad[:, -1] + 1) % P  # still canonical
        status = mm.verify_batch_many(root, dims, indices, bad, paths)
        assert (p3.host_u32(status) == p3.ROOT_MISMATCH).all(), tag


def _run_plain(p3, oracle, hash_name, cases, openings, profiles=mc.PROFILES):
    mm = p3.MerkleTreeMmcs(hash=hash_name)
    assert p3.get_thread_profile() == "latency"
    try:
        for case_id, dims in cases:
            mats = mc.matrices(case_id, dims)
            oroot, otree, olayers = _oracle_tree(oracle, mats, hash_name)
            for profile in profiles:
                p3.set_thread_profile(profile)
                root, tree = _commit(p3, mm, mats)
                tag = (hash_name, profile, case_id)
                _same_tree(root, tree, oroot, olayers, tag)
                if openings:
                    _openings(p3, mm, tree, root, otree, dims, case_id, tag)
                tree.free()
    finally:
        p3.set_thread_profile("latency")


# ---------------------------------------------------------------- A: one injected matrix at every level
@pytest.mark.parametrize("log_h", mc.GRID_A_LOG_HEIGHTS)
@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_one_injection_at_every_level(p3, oracle, hash_name, log_h):
    """[(2^H, 3), (2^j, 5)] for every j < H: an injection right after, right before and inside every fused run of levels"""
    _run_plain(p3, oracle, hash_name, mc.grid_a(log_h), openings=log_h in (13, 14, 16))


@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_a_layer_past_the_quad_forms_range(p3, oracle, hash_name):
    """2^17 rows: the one compression layer of 2^16 digests, which the latency profile too hands to compress_layer_f64_kernel"""
    _run_plain(p3, oracle, hash_name, mc.GRID_A_EXTRA, openings=True)


# ---------------------------------------------------------------- B: two injections, and all of them
@pytest.mark.parametrize("j1", range(mc.B_TOP - 1))
@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_two_injections_at_every_pair_of_levels(p3, oracle, hash_name, j1):
    cases = [(c, d) for c, d in mc.grid_b_pairs() if c.startswith("B-%d-" % j1)]
    assert len(cases) == mc.B_TOP - 1 - j1
    _run_plain(p3, oracle, hash_name, cases, openings=True)


@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_a_matrix_at_every_level_in_three_caller_orders(p3, oracle, hash_name):
    _run_plain(p3, oracle, hash_name, mc.grid_b_all(), openings=True)


# ---------------------------------------------------------------- C: class composition
@pytest.mark.parametrize("placement", ["leaf", "injected"])
@pytest.mark.parametrize("log_h", mc.C_CLASS_LOG_HEIGHTS)
@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_class_compositions(p3, oracle, hash_name, log_h, placement):
    """the cap of 16, the rate boundaries of both sponges, wide matrices alone and not alone, the salted shapes and their near-misses in
    a plain commitment, a zero-width matrix (accepted: an empty row hashes to the zero digest, include/p3hip.h) — as the leaf class
    and as an injected class, on both sides of the cooperative threshold"""
    cases = [(c, d) for c, d in mc.grid_c(log_h) if c.startswith("C-%d-%s-" % (log_h, placement))]
    assert len(cases) == len(mc.C_WIDTHS)
    _run_plain(p3, oracle, hash_name, cases, openings=True)


# ---------------------------------------------------------------- D: 64 matrices
@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_sixty_four_matrices(p3, oracle, hash_name):
    _run_plain(p3, oracle, hash_name, mc.grid_d(), openings=True)


# ---------------------------------------------------------------- hiding commitments
def _hiding_case(p3, oracle, hash_name, case_id, dims, profile):
    """MerkleTreeHidingMmcs, seed 1, against the oracle tree over the interleaved (matrix, salt) list; the salts from a host stream of
    the same seed, in input order"""
    mats = mc.matrices(case_id, dims)
    mmcs = p3.MerkleTreeHidingMmcs(hash_name, seed=1)
    host = oracle.rng_seed_from_u64(1)
    root, tree = mmcs.commit(mats)
    inter = []
    for m in mats:
        inter += [m, oracle.rng_fill_field(host, m.shape[0] * mc.SALT_ELEMS).reshape(m.shape[0], mc.SALT_ELEMS)]
    oroot, _, olayers = _oracle_tree(oracle, inter, hash_name)
    _same_tree(root, tree, oroot, olayers, (hash_name, profile, case_id, "hiding"))
    tree.free()


@pytest.mark.parametrize("log_h", mc.HIDING_LOG_HEIGHTS)
@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_hiding_classes(p3, oracle, hash_name, log_h):
    """classes of 1, 2, 4, 8 matrices of widths 4, 5, 6, 8: the salted<W,1> and salted<4,4> leaf kernels, the generic ones for every
    other combination, and the class cap filled by eight (matrix, salt) pairs"""
    try:
        for profile in mc.PROFILES:
            p3.set_thread_profile(profile)
            for case_id, dims in mc.grid_hiding(log_h):
                _hiding_case(p3, oracle, hash_name, case_id, dims, profile)
    finally:
        p3.set_thread_profile("latency")


@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_hiding_mixed_heights(p3, oracle, hash_name):
    try:
        for profile in mc.PROFILES:
            p3.set_thread_profile(profile)
            for case_id, dims in mc.HIDING_MIXED:
                _hiding_case(p3, oracle, hash_name, case_id, dims, profile)
    finally:
        p3.set_thread_profile("latency")


# ---------------------------------------------------------------- the caps
def _refused(p3, commit, mats, message):
    with pytest.raises(p3.P3HipError) as e:
        commit(mats)
    assert e.value.code == ERR_BAD_ARG and message in e.value.message, (e.value.code, e.value.message)


@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_refusals_leave_nothing_behind(p3, oracle, hash_name):
    """17 matrices of one height, 65 matrices, and for the hiding commit 9 of one height (18 leaf entries) and 33: P3HIP_ERR_BAD_ARG
    by name; a small commit afterwards still equals the oracle's — for the hiding MMCS with the SAME rng, whose stream a refused
    commit must not have advanced"""
    small = [("R-small", [(16, 3), (16, 2), (4, 5)])]
    mm = p3.MerkleTreeMmcs(hash=hash_name)
    _refused(p3, mm.commit, mc.matrices("R-17", [(8, 1)] * 17), "more than 16 matrices of one height")
    _refused(p3, mm.commit, mc.matrices("R-17-injected", [(16, 2)] + [(8, 1)] * 17), "more than 16 matrices of one height")
    _refused(p3, mm.commit, mc.matrices("R-65", [(1 << (k // 10), 1) for k in range(65)]), "at most 64 matrices per commitment")
    _run_plain(p3, oracle, hash_name, small, openings=True)
    _run_plain(p3, oracle, hash_name, [("R-16", [(8, 1)] * 16)], openings=True)  # the caps themselves are accepted

    mmcs = p3.MerkleTreeHidingMmcs(hash_name, seed=1)
    host = oracle.rng_seed_from_u64(1)
    _refused(p3, mmcs.commit, mc.matrices("R-h9", [(8, 2)] * 9), "more than 16 matrices of one height")
    _refused(p3, mmcs.commit, mc.matrices("R-h33", [(1 << (k // 8), 1) for k in range(33)]), "at most 32 matrices per commitment")
    for case_id, dims in small + [("R-h32", [(1 << (k // 8), 1 + k % 3) for k in range(32)])]:  # 32 matrices: 64 leaf entries, accepted
        mats = mc.matrices(case_id, dims)
        root, tree = mmcs.commit(mats)
        inter = []
        for m in mats:
            inter += [m, oracle.rng_fill_field(host, m.shape[0] * mc.SALT_ELEMS).reshape(m.shape[0], mc.SALT_ELEMS)]
        oroot, _, olayers = _oracle_tree(oracle, inter, hash_name)
        _same_tree(root, tree, oroot, olayers, (hash_name, case_id, "hiding, after the refusals"))
        tree.free()
