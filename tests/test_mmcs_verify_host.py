"""Mmcs::verify_batch of the product (p3hip_mmcs_verify_batch: host code, no GPU) against the oracle's: golden trees, seeded random
commitments of mixed heights (a height-1 matrix injected at the root, a commitment whose tallest height is 1), salted commitments
listed as m0, s0, m1, s1; every index or a seeded sample accepts, every single-word tamper of rows, path and root gets the oracle's
verdict, and so do a neighbouring index, swapped dims and the other hash configuration; the reject codes and the malformed calls."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden

P = 0x78000001
KINDS = (("poseidon2", 0), ("keccak", 1))
BAD_ARG = -1


def _rand(rng, h, w):
    return rng.integers(0, P, size=(h, w), dtype=np.uint64).astype(np.uint32)


def _raw(p3, kind, root, dims, index, rows, path, path_len=None, n_mats=None):
    """the C entry itself -> (return code, mailbox message)"""
    from plonky3_mobile_amd import _lib
    n = len(dims)
    hs = (C.c_size_t * max(n, 1))(*[d[0] for d in dims])
    ws = (C.c_size_t * max(n, 1))(*[d[1] for d in dims])
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    path = np.ascontiguousarray(path, dtype=np.uint32).reshape(-1, 8)
    root = np.ascontiguousarray(root, dtype=np.uint32)
    rc = _lib.lib().p3hip_mmcs_verify_batch(kind, root.ctypes.data_as(C.c_void_p), hs, ws, n if n_mats is None else n_mats, index,
                                            rows.ctypes.data_as(C.c_void_p), path.ctypes.data_as(C.c_void_p),
                                            path.shape[0] if path_len is None else path_len)
    return rc, _lib.take_last_error()


def _commitments():
    """(name, matrices) of every commitment under test"""
    out = []
    for k, t in enumerate(golden("mmcs.json")["trees"]):
        from oracle import oracle as o
        out.append(("golden%d" % k, [o.to_monty(np.array(m, dtype=np.uint64)).reshape(h, w) for m, (h, w) in zip(t["mats"], t["dims"])]))
    rng = np.random.default_rng(20251)
    for it in range(44):
        k = int(rng.integers(1, 5))
        dims = [(1 << int(rng.integers(0, 11)), int(rng.integers(1, 41))) for _ in range(k)]
        if it == 0:
            dims = [(1, 5)]                      # the tallest height is 1: path_len 0
        elif it == 1:
            dims = [(1, 3), (1, 40)]
        elif it in (2, 3):
            dims = dims[:3] + [(1, int(rng.integers(1, 41)))]  # a height-1 matrix, injected at the root
            if max(h for h, _ in dims) == 1:
                dims[0] = (64, dims[0][1])
        elif it == 4:
            dims = [(1 << 10, 40), (1 << 10, 1), (1 << 9, 17), (2, 8)]
        out.append(("random%d" % it, [_rand(rng, h, w) for h, w in dims]))
    for it in range(4):  # salted commitments as explicit m0, s0, m1, s1 lists (what the hiding MMCS commits to)
        k = int(rng.integers(1, 4))
        mats = []
        for _ in range(k):
            h = 1 << int(rng.integers(0, 9))
            mats += [_rand(rng, h, int(rng.integers(1, 20))), _rand(rng, h, 4)]
        out.append(("salted%d" % it, mats))
    return out


def _tamper(word, field, rng):
    if field:  # stays inside [0, P)
        return (int(word) + 1 + int(rng.integers(0, P - 1))) % P
    return int(word) ^ (1 << int(rng.integers(0, 32)))


@pytest.mark.parametrize("hash,kind", KINDS)
def test_verify_batch_agrees_with_the_oracle_on_honest_and_tampered_openings(p3, oracle, hash, kind):
    other = 1 - kind
    n_random = n_h1 = n_depth0 = 0
    for name, mats in _commitments():
        dims = [m.shape for m in mats]
        maxh = max(h for h, _ in dims)
        n_random += name.startswith("random")
        n_h1 += maxh > 1 and any(h == 1 for h, _ in dims)
        n_depth0 += maxh == 1
        root, tree = oracle.mmcs_commit(mats, kind)
        rng = np.random.default_rng(abs(hash_name(name)) + kind)
        indices = list(range(maxh)) if maxh <= 64 else sorted({0, maxh - 1} | {int(i) for i in rng.integers(0, maxh, 16)})
        mm = p3.MerkleTreeMmcs(hash)
        for idx in indices:
            rows, path = tree.open_batch(idx)
            assert oracle.mmcs_verify_batch(root, dims, idx, rows, path, kind), (name, idx)
            rc, msg = _raw(p3, kind, root, dims, idx, rows, path)
            assert rc == 0 and msg is None, (name, idx, rc, msg)
        idx = indices[int(rng.integers(0, len(indices)))]
        rows, path = tree.open_batch(idx)
        off, parts = 0, []
        for _, w in dims:
            parts.append(rows[off:off + w]); off += w
        assert mm.verify_batch(root, dims, idx, parts, path) is True
        # every single word of the rows, of the path and of the root, one at a time
        for what, arr, field in (("rows", rows, True), ("path", path.reshape(-1), kind == 0), ("root", root, kind == 0)):
            for k in range(arr.size):
                bad = arr.copy()
                bad[k] = _tamper(bad[k], field, rng)
                args = {"rows": rows, "path": path, "root": root}
                args[what] = bad
                exp = oracle.mmcs_verify_batch(args["root"], dims, idx, args["rows"], args["path"], kind)
                rc, msg = _raw(p3, kind, args["root"], dims, idx, args["rows"], args["path"])
                assert (rc == 0) == exp, (name, what, k, rc, msg)
                assert rc in (0, 1) and (rc == 0 or "RootMismatch" in msg), (name, what, k, rc, msg)
        bad_root = root.copy()
        bad_root[3] = _tamper(bad_root[3], kind == 0, rng)
        assert mm.verify_batch(bad_root, dims, idx, parts, path) is False
        # a neighbouring index, two matrices swapped in dims, the other hash configuration
        if maxh > 1:
            rc, _ = _raw(p3, kind, root, dims, idx ^ 1, rows, path)
            assert (rc == 0) == oracle.mmcs_verify_batch(root, dims, idx ^ 1, rows, path, kind), (name, "index ^ 1")
        if len(dims) > 1:
            a, b = (int(v) for v in rng.choice(len(dims), 2, replace=False))
            sw = list(dims)
            sw[a], sw[b] = sw[b], sw[a]
            rc, _ = _raw(p3, kind, root, sw, idx, rows, path)
            assert (rc == 0) == oracle.mmcs_verify_batch(root, sw, idx, rows, path, kind), (name, "swapped dims", sw)
        rows_o = rows
        path_o = path % P if other == 0 else path  # the Poseidon2 configuration takes canonical digest words only
        rc, _ = _raw(p3, other, root % P if other == 0 else root, dims, idx, rows_o, path_o)
        assert (rc == 0) == oracle.mmcs_verify_batch(root % P if other == 0 else root, dims, idx, rows_o, path_o, other), (name, "other hash")
    assert n_random >= 40 and n_h1 >= 2 and n_depth0 >= 2


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


@pytest.mark.parametrize("hash,kind", KINDS)
def test_verify_batch_reject_codes(p3, oracle, hash, kind):
    rng = np.random.default_rng(5)
    mats = [_rand(rng, 64, 5), _rand(rng, 16, 9), _rand(rng, 1, 2)]
    dims = [m.shape for m in mats]
    root, tree = oracle.mmcs_commit(mats, kind)
    idx = 37
    rows, path = tree.open_batch(idx)
    mm = p3.MerkleTreeMmcs(hash)
    parts = [rows[:5], rows[5:14], rows[14:]]
    assert _raw(p3, kind, root, dims, idx, rows, path)[0] == 0
    # a wrong path length: 2
    for pl, pth in ((5, path[:5]), (7, np.concatenate([path, path[:1]]))):
        rc, msg = _raw(p3, kind, root, dims, idx, rows, pth)
        assert rc == 2 and "WrongHeight" in msg
    with pytest.raises(ValueError, match="WrongHeight"):
        mm.verify_batch(root, dims, idx, parts, path[:5])
    # a row word that is no canonical field element: 3, whichever matrix holds it
    for k in (0, 4, 5, 13, 15):
        for v in (P, P + 1, 0xffffffff):
            bad = rows.copy()
            bad[k] = v
            rc, msg = _raw(p3, kind, root, dims, idx, bad, path)
            assert rc == 3 and "canonical" in msg, (k, v, rc)
    with pytest.raises(ValueError, match="canonical"):
        mm.verify_batch(root, dims, idx, [np.array([P] * 5, np.uint32)] + parts[1:], path)
    # a digest word >= P: refused under Poseidon2, hashed under Keccak (a [u64; 4] digest has no such rule)
    for k in (0, 7, 8 * 3 + 2, path.size - 1):
        bad = path.copy().reshape(-1)
        bad[k] = P if kind == 0 else (0xffffffff if int(bad[k]) != 0xffffffff else 0xfffffffe)
        rc, msg = _raw(p3, kind, root, dims, idx, rows, bad)
        assert rc == (3 if kind == 0 else 1), (k, rc, msg)
        if kind == 1:
            assert not oracle.mmcs_verify_batch(root, dims, idx, rows, bad.reshape(-1, 8), kind)
    if kind == 1:  # honest Keccak digests do have words >= P, and they verify
        assert (path >= P).any() or (root >= P).any()
    # index = the tallest height: 4
    for bad_idx in (64, 65, 1 << 40):
        rc, msg = _raw(p3, kind, root, dims, bad_idx, rows, path)
        assert rc == 4 and "index" in msg
    with pytest.raises(ValueError, match="index"):
        mm.verify_batch(root, dims, 64, parts, path)


def test_verify_batch_malformed_calls(p3, oracle):
    from plonky3_mobile_amd import _lib
    rng = np.random.default_rng(6)
    mats = [_rand(rng, 8, 3), _rand(rng, 4, 2)]
    dims = [m.shape for m in mats]
    root, tree = oracle.mmcs_commit(mats)
    rows, path = tree.open_batch(5)
    L = _lib.lib()
    hs, ws = (C.c_size_t * 2)(8, 4), (C.c_size_t * 2)(3, 2)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [0, vp(root), hs, ws, 2, 5, vp(rows), vp(path), 3]
    assert L.p3hip_mmcs_verify_batch(*good) == 0 and _lib.take_last_error() is None
    for pos in (1, 2, 3, 6, 7):  # a null pointer
        args = list(good)
        args[pos] = None
        assert L.p3hip_mmcs_verify_batch(*args) == BAD_ARG, pos
        assert "null" in _lib.take_last_error()
    big = (C.c_size_t * 65)(*([8] * 65))
    one = (C.c_size_t * 65)(*([1] * 65))
    for args, word in (([0, vp(root), hs, ws, 0, 5, vp(rows), vp(path), 3], "no matrices"),
                       ([0, vp(root), big, one, 65, 5, vp(np.zeros(65, np.uint32)), vp(path), 3], "at most 64"),
                       ([0, vp(root), (C.c_size_t * 2)(8, 3), ws, 2, 5, vp(rows), vp(path), 3], "powers of two"),
                       ([0, vp(root), (C.c_size_t * 2)(8, 0), ws, 2, 5, vp(rows), vp(path), 3], "powers of two"),
                       ([7, vp(root), hs, ws, 2, 5, vp(rows), vp(path), 3], "unknown hash")):
        assert L.p3hip_mmcs_verify_batch(*args) == BAD_ARG, word
        msg = _lib.take_last_error()
        assert msg and word in msg, (word, msg)
    with pytest.raises(p3.P3HipError):
        p3.MerkleTreeMmcs().verify_batch(root, [(8, 3), (3, 2)], 5, [rows[:3], rows[3:]], path)
    # 64 matrices is the limit, not beyond it
    mats64 = [_rand(rng, 2, 1) for _ in range(64)]
    r64, t64 = oracle.mmcs_commit(mats64)
    rows64, path64 = t64.open_batch(1)
    assert _raw(p3, 0, r64, [m.shape for m in mats64], 1, rows64, path64)[0] == 0


@pytest.mark.parametrize("hash,kind", KINDS)
def test_hiding_verify_batch_takes_values_and_salts(p3, oracle, hash, kind):
    """MerkleTreeHidingMmcs.verify_batch merges (values, (salts, siblings)) into the m0, s0, m1, s1 row the tree was built on."""
    rng = np.random.default_rng(9)
    vals = [_rand(rng, 32, 6), _rand(rng, 8, 3)]
    salts = [_rand(rng, 32, 4), _rand(rng, 8, 4)]
    inter = [vals[0], salts[0], vals[1], salts[1]]
    root, tree = oracle.mmcs_commit(inter, kind)
    mm = p3.MerkleTreeHidingMmcs(hash)  # no rng is created: verification is host code
    for idx in (0, 13, 31):
        ov = [vals[0][idx], vals[1][idx >> 2]]
        os_ = [salts[0][idx], salts[1][idx >> 2]]
        path = tree.open_batch(idx)[1]
        assert mm.verify_batch(root, [(32, 6), (8, 3)], idx, ov, (os_, path)) is True
        bad = [s.copy() for s in os_]
        bad[1][2] = (int(bad[1][2]) + 1) % P
        assert mm.verify_batch(root, [(32, 6), (8, 3)], idx, ov, (bad, path)) is False


def test_cpp_mirror_verify_batch_compiles(tmp_path):
    """include/p3hip.hpp: a translation unit that calls MerkleTreeMmcs::verify_batch and the two bulk wrappers compiles."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / "vb.cpp"
    src.write_text('#include "p3hip.hpp"\n'
                   "bool f(const std::vector<uint32_t>& root, const std::vector<std::vector<uint32_t>>& rows, const std::vector<uint32_t>& path,\n"
                   "       const p3hip::MerkleTree& t, const uint32_t* di, uint32_t* dr, uint32_t* dp, uint32_t* ds) {\n"
                   "    p3hip::MerkleTreeMmcs mm(P3HIP_HASH_KECCAK);\n"
                   "    mm.open_batch_many_dev(t, di, 4, dr, dp);\n"
                   "    mm.verify_batch_many_dev(root, {{8, 3}, {4, 2}}, di, 4, dr, dp, ds);\n"
                   "    return mm.row_words(t) == 5 && mm.verify_batch(root, {{8, 3}, {4, 2}}, 5, rows, path);\n"
                   "}\n"
                   "int main() { return P3HIP_MMCS_ROOT_MISMATCH + P3HIP_MMCS_WRONG_HEIGHT + P3HIP_MMCS_NOT_CANONICAL + P3HIP_MMCS_BAD_INDEX == 10 ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cpp_mirror_verify_batch_runs(p3, oracle, tmp_path):
    """the same mirror linked against the library: accept, RootMismatch -> false, a reject with its message thrown"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    rng = np.random.default_rng(12)
    mats = [_rand(rng, 8, 3), _rand(rng, 4, 2)]
    root, tree = oracle.mmcs_commit(mats)
    rows, path = tree.open_batch(5)
    lit = lambda a: "{" + ", ".join("%du" % int(v) for v in np.asarray(a).reshape(-1)) + "}"
    src = tmp_path / "vbrun.cpp"
    src.write_text('#include <cstdio>\n#include "p3hip.hpp"\n'
                   "int main() {\n"
                   "    p3hip::MerkleTreeMmcs mm;\n"
                   "    std::vector<uint32_t> root = %s, path = %s;\n"
                   "    std::vector<std::vector<uint32_t>> rows = {%s, %s};\n"
                   "    if (!mm.verify_batch(root, {{8, 3}, {4, 2}}, 5, rows, path)) return 1;\n"
                   "    if (mm.verify_batch(root, {{8, 3}, {4, 2}}, 4, rows, path)) return 2;\n"
                   "    try { mm.verify_batch(root, {{8, 3}, {4, 2}}, 8, rows, path); return 3; }\n"
                   '    catch (const p3hip::Error& e) { if (e.code != P3HIP_MMCS_BAD_INDEX) return 4; std::puts(e.what()); }\n'
                   "    return 0;\n}\n" % (lit(root), lit(path), lit(rows[:3]), lit(rows[3:])))
    libdir = os.path.dirname(p3._lib.LIB_PATH)
    exe = tmp_path / "vbrun"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lp3hip",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "index" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_verify_kernels_use_no_scratch():
    """The device forms keep every state in registers: compiled with the resource report, each kernel of mmcs_verify.hip, the
    bulk gather of mmcs.hip and every instantiation of the batch verifiers' opening kernel (the same per-lane walk, lane_walk.hip.h)
    show 0 bytes of scratch per lane."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "plonky3-mobile_amd", "csrc")
    instances = {"pv_open_kernel": 4}  # per hash and (one height / mixed heights)
    for src, kernels in (("mmcs_verify.hip", ("verify_lane_p2_kernel", "verify_lane_keccak_kernel", "verify_coop_p2_kernel", "verify_coop_keccak_kernel")),
                         ("mmcs.hip", ("open_gather_many_kernel",)),
                         ("pcs_verifier_dev.hip", ("pv_open_kernel",))):
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, src), "-o", os.devnull], capture_output=True, text=True, cwd=csrc)
        assert r.returncode == 0, r.stderr[-2000:]
        found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, flags=re.S)
        for k in kernels:
            hit = [int(sz) for n, sz in found if k in n]
            assert len(hit) >= instances.get(k, 1) and all(v == 0 for v in hit), (k, hit)


def test_host_verifiers_keep_their_codes_on_non_canonical_words(p3, oracle):
    """The proof verifiers share Mmcs::verify_batch but hash an opening's words as their reader hands them over: a proof in which
    one word w is replaced by w + P (the same value, not canonical) gets the reject code and message it always got, for every
    such word of a plain and a hiding proof under both hash configurations (recorded before the sharing: tests/golden)."""
    g = golden("verifier_noncanonical_codes.json")["cases"]
    t, log_n = (1, 0, 10, 4), 3
    ofp, gfp = oracle.FriParams(*t), p3.FriParameters(*t)
    x = oracle.fib_public_x(0, 1, 8)
    # words accepted as their value and flagged by the reader afterwards (9), and openings refused (13, 14), all occur
    assert {r[1] for c in g.values() for r in c["results"]} >= {9, 13, 14}
    for hash, kind in KINDS:
        for hiding in (False, True):
            proof = (oracle.prove_fib_air_hiding if hiding else oracle.prove_fib_air)(0, 1, log_n, ofp, hash=kind)
            w = np.frombuffer(proof, np.uint32)
            case = g["%s_%s" % (hash, "hiding" if hiding else "plain")]
            assert [r[0] for r in case["results"]] == [k for k in range(len(w)) if w[k] < P and int(w[k]) + P < 2 ** 32]
            for pos, code, m in case["results"]:
                bad = w.copy()
                bad[pos] = int(w[pos]) + P
                with pytest.raises(p3.P3HipError) as e:
                    p3.verify_fib_air(bad.tobytes(), 0, 1, x, log_n, gfp, hash=hash, hiding=hiding)
                assert (e.value.code, e.value.message) == (code, case["messages"][m]), (hash, hiding, pos)
