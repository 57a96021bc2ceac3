"""The bulk, device-resident halves of the MMCS contract on the GPU: open_batch_many against the per-index open_batch and the
oracle's, verify_batch_many against the oracle's verdicts on honest and tampered openings, every per-opening code, both kernel
forms (one opening per lane; lane-cooperative for small n), the sizes users run, one stream without a host touch, and lifetime.
Both hash configurations, both thread profiles, plain and hiding trees."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0x78000001
MIB = 1 << 20
HASHES = ["poseidon2", "keccak"]
LANE, COOP = 1, 2


def _rand(rng, h, w):
    return rng.integers(0, P, size=(h, w), dtype=np.uint64).astype(np.uint32)


def _kind(oracle, hash):
    return oracle.HASH_KECCAK if hash == "keccak" else oracle.HASH_POSEIDON2


def _indices(rng, maxh, n):
    idx = rng.integers(0, maxh, n).astype(np.uint32)
    idx[0] = 0
    idx[-1] = maxh - 1
    if n > 3:
        idx[n // 2] = idx[1]  # a duplicate
    return idx


def _oracle_status(oracle, root, dims, idx, rows, paths, kind):
    return np.array([0 if oracle.mmcs_verify_batch(root, dims, int(i), r, p, kind) else 1 for i, r, p in zip(idx, rows, paths)], np.uint32)


def _tamper_quarter(rng, rows, paths, field_paths):
    """one seeded word in a seeded quarter of the openings, rows and paths alternately (rows only when there is no path) -> which"""
    rows, paths = rows.copy(), paths.copy()
    n = rows.shape[0]
    pick = rng.choice(n, size=max(1, n // 4), replace=False)
    for j, i in enumerate(pick):
        in_path = bool(j % 2 and paths[i].size)
        tgt = paths[i].reshape(-1) if in_path else rows[i]
        k = int(rng.integers(0, tgt.size))
        if not in_path or field_paths:
            tgt[k] = (int(tgt[k]) + 1 + int(rng.integers(0, P - 1))) % P
        else:
            tgt[k] = int(tgt[k]) ^ (1 << int(rng.integers(0, 32)))
    return rows, paths, np.sort(pick)


def _status(p3, mm, root, dims, idx, rows, paths, form=0):
    st, rej = mm._verify_many(root, dims, p3.dev_u32(idx), p3.dev_u32(rows), p3.dev_u32(paths), form, True)
    return p3.host_u32(st), int(p3.host_u32(rej)[0])


@pytest.mark.parametrize("profile", ["latency", "throughput"])
@pytest.mark.parametrize("hash", HASHES)
def test_bulk_open_and_verify_on_random_commitments(p3, oracle, hash, profile):
    kind = _kind(oracle, hash)
    rng = np.random.default_rng(4242 + kind)
    p3.set_thread_profile(profile)
    try:
        mm = p3.MerkleTreeMmcs(hash)
        mmh = p3.MerkleTreeHidingMmcs(hash, seed=1)
        host_rng = oracle.rng_seed_from_u64(1)
        for it in range(30):
            k = int(rng.integers(1, 5))
            dims = [(1 << int(rng.integers(0, 12)), int(rng.integers(1, 49))) for _ in range(k)]
            if it == 0:
                dims = [(1, 7)]
            if it == 1:
                dims = [(256, 48), (256, 1), (1, 5)]
            mats = [_rand(rng, h, w) for h, w in dims]
            hiding = it % 3 == 2
            if hiding:
                root, tree = mmh.commit(mats)
                full = []
                for m in mats:
                    full += [m, oracle.rng_fill_field(host_rng, m.shape[0] * 4).reshape(m.shape[0], 4)]
            else:
                root, tree = mm.commit(mats)
                full = mats
            fdims = [m.shape for m in full]
            oroot, otree = oracle.mmcs_commit(full, kind)
            assert np.array_equal(root, oroot), (it, dims)
            maxh, depth = max(h for h, _ in dims), tree.log_max_height
            single = {}
            for n in (1, 63, 64, 65, 1000):
                idx = _indices(rng, maxh, n)
                if hiding:
                    vals, (salts, paths_d) = mmh.open_batch_many(idx, tree)
                    assert vals.shape == (n, sum(w for _, w in dims)) and salts.shape == (n, len(mats), 4)
                    rows_d, _ = mmh._open_many(idx, tree)
                else:
                    rows_d, paths_d = mm.open_batch_many(idx, tree)
                rows, paths = p3.host_u32(rows_d), p3.host_u32(paths_d)
                assert rows.shape == (n, sum(w for _, w in fdims)) and paths.shape == (n, depth, 8)
                for j, i in enumerate(idx):
                    i = int(i)
                    if i not in single:
                        orows, opath = otree.open_batch(i)
                        if hiding:
                            v, (s, pth) = mmh.open_batch(i, tree)
                            got = np.concatenate([np.concatenate([a, b]) for a, b in zip(v, s)])
                        else:
                            r, pth = mm.open_batch(i, tree)
                            got = np.concatenate(r)
                        assert np.array_equal(got, orows) and np.array_equal(pth, opath), (it, dims, i)
                        single[i] = (orows, opath)
                    assert np.array_equal(rows[j], single[i][0]) and np.array_equal(paths[j], single[i][1]), (it, dims, n, j, i)
                # honest openings: all 0
                if hiding:
                    st, rej = mmh.verify_batch_many(root, dims, idx, vals, (salts, paths_d), with_rejected=True)
                    st, rej = p3.host_u32(st), int(p3.host_u32(rej)[0])
                else:
                    st, rej = _status(p3, mm, root, fdims, idx, rows, paths)
                assert not st.any() and rej == 0, (it, dims, n, st.nonzero())
                # one seeded word tampered in a seeded quarter: the oracle's verdict, opening by opening
                trows, tpaths, pick = _tamper_quarter(rng, rows, paths, kind == 0)
                exp = _oracle_status(oracle, root, fdims, idx, trows, tpaths, kind)
                assert np.array_equal(np.flatnonzero(exp), pick)
                for form in (0, LANE, COOP):
                    st, rej = _status(p3, mm, root, fdims, idx, trows, tpaths, form)
                    assert np.array_equal(st, exp) and rej == int(exp.sum()), (it, dims, n, form)
                # a wrong root rejects all of them
                bad_root = root.copy()
                bad_root[5] = (int(bad_root[5]) + 1) % P if kind == 0 else int(bad_root[5]) ^ 4
                st, rej = _status(p3, mm, bad_root, fdims, idx, rows, paths)
                assert (st == 1).all() and rej == n
            tree.free()
    finally:
        p3.set_thread_profile("latency")


@pytest.mark.parametrize("form", [LANE, COOP])
@pytest.mark.parametrize("hash", HASHES)
def test_every_per_opening_code_from_the_device(p3, oracle, hash, form):
    kind = _kind(oracle, hash)
    rng = np.random.default_rng(31 + kind)
    mats = [_rand(rng, 512, 11), _rand(rng, 64, 3), _rand(rng, 1, 2)]
    dims = [m.shape for m in mats]
    mm = p3.MerkleTreeMmcs(hash)
    root, tree = mm.commit(mats)
    n = 200
    idx = _indices(rng, 512, n)
    rows_d, paths_d = mm.open_batch_many(idx, tree)
    rows, paths = p3.host_u32(rows_d).copy(), p3.host_u32(paths_d).copy()
    exp = np.zeros(n, np.uint32)
    rows[3, 0] = P; exp[3] = 3                # a row word >= P, in each matrix
    rows[70, 12] = 0xffffffff; exp[70] = 3
    rows[64, 15] = P + 5; exp[64] = 3
    if kind == 0:
        paths[9, 0, 0] = P; exp[9] = 3        # a Poseidon2 digest word >= P
        paths[130, 8, 7] = 0xfffffffe; exp[130] = 3
    else:                                     # a Keccak digest word >= P is hashed, not refused
        paths[9, 0, 0] = 0xffffffff if paths[9, 0, 0] != 0xffffffff else 0xfffffffe; exp[9] = 1
    idx = idx.copy()
    idx[20] = 512; exp[20] = 4                # an index >= the tallest height
    idx[199] = 0xffffffff; exp[199] = 4
    idx[63] = 512 + int(idx[63]); exp[63] = 4
    rows[199, 1] = P                          # out of range AND not canonical: the index decides, as on the host
    st, rej = _status(p3, mm, root, dims, idx, rows, paths, form)
    assert np.array_equal(st, exp), np.flatnonzero(st != exp)
    assert rej == int((exp != 0).sum())
    for i in (2, 4, 8, 10, 19, 21, 62, 65, 69, 71, 198):  # their neighbours are still 0
        assert st[i] == 0
    tree.free()


@pytest.mark.parametrize("profile", ["latency", "throughput"])
@pytest.mark.parametrize("hash", HASHES)
def test_both_forms_give_the_same_statuses(p3, oracle, hash, profile):
    """Each form on leaf widths around the absorb blocks (8 words under Poseidon2, 34 under Keccak) and at depth 0; n on either side
    of the crossover constant of this hash and profile."""
    from plonky3_mobile_amd import _lib
    kind = _kind(oracle, hash)
    rng = np.random.default_rng(77 + kind)
    mm = p3.MerkleTreeMmcs(hash)
    p3.set_thread_profile(profile)
    try:
        for w in (1, 7, 8, 9, 16, 34, 35, 68):
            for dims in ([(128, w)], [(1, w)], [(32, w), (32, 3), (4, w)]):
                mats = [_rand(rng, h, ww) for h, ww in dims]
                root, tree = mm.commit(mats)
                oroot, _ = oracle.mmcs_commit(mats, kind)
                assert np.array_equal(root, oroot)
                n = 150
                idx = _indices(rng, dims[0][0], n)
                rows_d, paths_d = mm.open_batch_many(idx, tree)
                rows, paths = p3.host_u32(rows_d), p3.host_u32(paths_d)
                trows, tpaths, _ = _tamper_quarter(rng, rows, paths, kind == 0)
                exp = _oracle_status(oracle, root, dims, idx, trows, tpaths, kind)
                for form in (LANE, COOP):
                    st, rej = _status(p3, mm, root, dims, idx, rows, paths, form)
                    assert not st.any() and rej == 0, (w, dims, form)
                    st, rej = _status(p3, mm, root, dims, idx, trows, tpaths, form)
                    assert np.array_equal(st, exp) and rej == int(exp.sum()), (w, dims, form)
                tree.free()
        cmax = _lib.lib().p3hip_mmcs_verify_coop_max(kind, 2 if profile == "latency" else 1)
        assert cmax == _lib.lib().p3hip_mmcs_verify_coop_max(kind, 2) // (1 if profile == "latency" else 4)
        mats = [_rand(rng, 1 << 12, 5), _rand(rng, 1 << 7, 9)]
        dims = [m.shape for m in mats]
        root, tree = mm.commit(mats)
        for n in sorted({max(cmax, 1), cmax + 1, 2 * cmax + 3}):
            idx = _indices(rng, 1 << 12, n)
            rows_d, paths_d = mm.open_batch_many(idx, tree)
            rows, paths = p3.host_u32(rows_d), p3.host_u32(paths_d)
            trows, tpaths, pick = _tamper_quarter(rng, rows, paths, kind == 0)
            exp = np.zeros(n, np.uint32)
            exp[pick] = 1
            sample = rng.choice(n, size=min(n, 200), replace=False)
            assert np.array_equal(_oracle_status(oracle, root, dims, idx[sample], trows[sample], tpaths[sample], kind), exp[sample])
            got = [_status(p3, mm, root, dims, idx, trows, tpaths, form) for form in (0, LANE, COOP)]
            for st, rej in got:
                assert np.array_equal(st, exp) and rej == len(pick), (n, cmax)
        tree.free()
    finally:
        p3.set_thread_profile("latency")


@pytest.mark.parametrize("profile", ["latency", "throughput"])
@pytest.mark.parametrize("hash", HASHES)
def test_the_sizes_users_run(p3, oracle, hash, profile):
    """The cfg2 trace commitment (2^21 x 2): one proof's 100 queries, and 2^16 seeded indices checked against the oracle in full; an
    FRI-layer shape (2^20 x 8); the cfg5 shape (2^16 x 2633), 256 openings."""
    import torch
    kind = _kind(oracle, hash)
    rng = np.random.default_rng(2100 + kind)
    mm = p3.MerkleTreeMmcs(hash)
    p3.set_thread_profile(profile)
    try:
        _sizes(p3, oracle, mm, kind, rng)
    finally:
        p3.set_thread_profile("latency")


def _sizes(p3, oracle, mm, kind, rng):
    import torch
    for h, w, ns in ((1 << 21, 2, (100, 1 << 16)), (1 << 20, 8, (100, 4096)), (1 << 16, 2633, (256,))):
        m = torch.randint(0, P, (h, w), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(h + w))
        root, tree = mm.commit([m])
        dims = [(h, w)]
        for n in ns:
            idx = _indices(rng, h, n)
            rows_d, paths_d = mm.open_batch_many(idx, tree)
            assert torch.equal(rows_d, m[torch.from_numpy(idx.astype(np.int64)).cuda()])
            st, rej = mm.verify_batch_many(root, dims, idx, rows_d, paths_d, with_rejected=True)
            assert not p3.host_u32(st).any() and int(p3.host_u32(rej)[0]) == 0, (h, w, n)
            assert not p3.host_u32(mm.verify_batch_many(root, dims, idx, rows_d, paths_d)).any()  # d_rejected = NULL: no counter
            rows, paths = p3.host_u32(rows_d), p3.host_u32(paths_d)
            trows, tpaths, pick = _tamper_quarter(rng, rows, paths, kind == 0)
            full = n == 1 << 16 or n <= 256
            sample = np.arange(n) if full else rng.choice(n, size=256, replace=False)
            exp = np.zeros(n, np.uint32)
            exp[pick] = 1
            assert np.array_equal(_oracle_status(oracle, root, dims, idx[sample], trows[sample], tpaths[sample], kind), exp[sample]), (h, w, n)
            for form in (0, LANE) + ((COOP,) if n <= 4096 else ()):
                st, rej = _status(p3, mm, root, dims, idx, trows, tpaths, form)
                assert np.array_equal(st, exp) and rej == len(pick), (h, w, n, form)
        tree.free()
        del m


def _chain(L, kind, stream, d_mat, h, w, d_layers, root, d_idx, n, d_rows, d_paths, d_status, d_rej):
    """commit -> open n indices -> verify them, enqueued back to back; returns the tree handle (host object only)"""
    from plonky3_mobile_amd import _lib
    ptrs = (C.c_void_p * 1)(d_mat.data_ptr())
    hs, ws = (C.c_size_t * 1)(h), (C.c_size_t * 1)(w)
    tree = C.c_void_p()
    sp = C.c_void_p(stream.cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.p3hip_mmcs_commit_into_dev(kind, ptrs, hs, ws, 1, vp(d_layers), C.byref(tree), sp))
    _lib.check(L.p3hip_mmcs_open_batch_many_dev(tree, vp(d_idx), n, vp(d_rows), vp(d_paths), sp))
    _lib.check(L.p3hip_mmcs_verify_batch_many_dev(kind, root.ctypes.data_as(C.c_void_p), hs, ws, 1, vp(d_idx), n, vp(d_rows), vp(d_paths),
                                                  vp(d_status), vp(d_rej), sp))
    return tree


def _chain_buffers(p3, oracle, hash, h, w, n, seed):
    import torch
    from plonky3_mobile_amd import _lib
    L = _lib.lib()
    kind = _kind(oracle, hash)
    rng = np.random.default_rng(seed)
    m = _rand(rng, h, w)
    root, _ = oracle.mmcs_commit([m], kind)  # the verifier knows the commitment: nothing comes back from the device before the end
    depth = h.bit_length() - 1
    idx = _indices(rng, h, n)
    idx[7] = h + 3  # one opening the device must refuse: masked by the gather, out of range for the verifier
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    bufs = dict(d_mat=p3.dev_u32(m), h=h, w=w, d_layers=z(L.p3hip_mmcs_layer_words(h)), root=root, d_idx=p3.dev_u32(idx), n=n,
                d_rows=z(n, w), d_paths=z(n, depth, 8), d_status=z(n), d_rej=z(1))
    return L, kind, bufs


@pytest.mark.parametrize("hash", HASHES)
def test_commit_open_verify_on_one_stream_without_a_host_touch(p3, oracle, hash):
    import torch
    L, kind, b = _chain_buffers(p3, oracle, hash, 1 << 14, 6, 3000, 5)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    tree = _chain(L, kind, stream, **b)
    stream.synchronize()                     # the one synchronise
    st = p3.host_u32(b["d_status"])          # the one download
    exp = np.zeros(b["n"], np.uint32)
    exp[7] = 4
    assert np.array_equal(st, exp)
    assert int(p3.host_u32(b["d_rej"])[0]) == 1
    L.p3hip_mmcs_free(tree)


def test_the_chain_allocates_nothing(p3, oracle):
    """25 repetitions of commit -> open -> verify (both hashes, both forms by n) leave the card's free memory where the warm-up
    repetitions left it: the method of test_gpu_lifetime.py."""
    import torch
    sets = [_chain_buffers(p3, oracle, hash, 1 << 13, 5, n, 8 + n) for hash in HASHES for n in (100, 9000)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def cycle():
        for L, kind, b in sets:
            tree = _chain(L, kind, stream, **b)
            stream.synchronize()
            assert int(p3.host_u32(b["d_rej"])[0]) == 1
            L.p3hip_mmcs_free(tree)
        gc.collect()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    for _ in range(3):
        cycle()
    base = free_bytes()
    for _ in range(25):
        cycle()
    lost = base - free_bytes()
    # these calls allocate nothing; one leaked row, path or layer buffer per repetition would cost > 25 x 0.3 MiB
    assert lost < 1 * MIB, "free device memory fell by %.2f MiB over 25 repetitions" % (lost / MIB)
