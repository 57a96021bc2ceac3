"""GPU tests of p2f::internal_rounds with dyadic lanes (csrc/poseidon2_f64.hip.h) through the existing fp64 probe
(p3hip_poseidon2_f64_probe_dev, mode 1: the thirteen internal rounds; mode 0: the whole permutation), against big-integer arithmetic,
and Merkle commits through the public entry, one of them under the throughput profile so that leaf_hash_f64_kernel runs the same
code.  A few thousand states in all; the entry sets and the fold-edge family come from tests/poseidon2_dyadic_ref.py (tests/test_poseidon2_dyadic_host.py shows, on the CPU, that the
fold-edge entries reach their folds on the fractional parts they are named for)."""
import ctypes as C

import numpy as np
import pytest

import field_ref as F
import poseidon2_dyadic_ref as D
import poseidon2_sched_ref as S

pytestmark = pytest.mark.gpu
P = D.P


def _probe(p3, entries, mode):
    """integer-valued doubles in, canonical values out: (n, 16) lists of integers in [0, P)"""
    import torch
    from plonky3_mobile_amd import _lib
    arr = np.array(entries, dtype=np.float64)
    assert arr.ndim == 2 and arr.shape[1] == 16 and arr.shape[0] <= 1 << 12
    assert all(int(a) == b for a, b in zip(arr.reshape(-1).tolist(), (v for e in entries for v in e)))  # exactly representable
    d = torch.from_numpy(arr).cuda()
    out = torch.empty(d.shape, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().p3hip_poseidon2_f64_probe_dev(C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), d.shape[0], mode,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return F.v_canon(out.cpu().numpy().view(np.uint32)).tolist()


def _check_rounds(p3, entries):
    got = _probe(p3, entries, 1)
    for e, row in zip(entries, got):
        assert row == D.reference_rounds(e), e


def test_sign_patterns_at_every_magnitude_and_single_lanes(p3):
    """all +, all -, signs of V, -signs of V, alternating at P - 1, 35 (P/2 + 2^9) and 2^37 - 1; zeros; +-(2^37 - 1) on one lane"""
    _check_rounds(p3, D.pattern_entries())


def test_seam3_family_entries(p3):
    """the 103 targets of the seam-3 family as the internal rounds see them (one external layer of y); and the family's seam-3 states
    through the whole permutation (mode 0), against pyref's permutation computed once for the family"""
    _check_rounds(p3, D.seam3_entries())
    idx = [j for j, f in enumerate(S.family()) if f[1] == 3]
    got = _probe(p3, [S.family()[j][3] for j in idx], 0)
    assert got == S.family_expected()[idx].tolist()


def test_random_entries_in_a_ragged_grid(p3):
    """1000 seeded entries up to 2^37 - 1: 3 workgroups of 256 and a last one of 232 lanes, 40 of them in its last wave"""
    ents = D.random_entries(1000, 21)
    assert len(ents) % 64 == 40
    _check_rounds(p3, ents)


def test_fold_edges(p3):
    """Every dyadic lane at its first fold with fractional part 0, 2^-F and 1 - 2^-F, the dyadic partial sum with 0 and 1 - 2^-F (rounds
    1 and 7), each with a positive and a negative value: fract of a negative number is where x - fract(x) P would go wrong."""
    fe = D.fold_edge_entries()
    assert len(fe) == 50
    got = _probe(p3, [f[5] for f in fe], 1)
    for (what, lane, r, want, sign, e), row in zip(fe, got):
        assert row == D.reference_rounds(e), (what, lane, r, want, sign)


def test_whole_family_through_the_whole_permutation(p3):
    """all 824 family states (every target at every seam) in probe mode 0 against pyref's permutation, computed once for the family"""
    fam = S.family()
    assert len(fam) == 824
    assert _probe(p3, [f[3] for f in fam], 0) == S.family_expected().tolist()


@pytest.mark.parametrize("log_h,profile", [(7, "latency"), (12, "throughput")])
def test_commit_layer_by_layer(p3, oracle, log_h, profile):
    """One commit of a 2^7 x 2 matrix through the public entry (under the default thread profile), every layer against the oracle.  A
    tree that small is hashed by the lane-cooperative kernels, which do not call p2f::permute, and under the default (latency) profile
    rows up to 2^15 go to the quad form.  The layer kernels that run the changed rounds are reached under the THROUGHPUT profile, the
    one the benchmark's provers use: there a 2^12 x 2 commit hashes its rows with leaf_hash_f64_kernel (its layers of 2^11 digests
    and fewer are cooperative again).  compress_layer_f64_kernel is reached by compressing that tree's leaf digests once more through
    form 1 of compress_layer_variant.  All must give the oracle's layers."""
    import torch
    rng = np.random.default_rng([F.SEED, 22, log_h])
    m = rng.integers(0, P, size=(1 << log_h, 2), dtype=np.uint64).astype(np.uint32)
    m[0] = 0
    m[1] = P - 1
    oroot, otree = oracle.mmcs_commit([m])
    olayers = otree.layers()
    assert p3.get_thread_profile() == "latency"
    try:
        p3.set_thread_profile(profile)
        root, tree = p3.MerkleTreeMmcs().commit([m])
        layers = tree.digest_layers()
        tree.free()
    finally:
        p3.set_thread_profile("latency")
    assert len(layers) == len(olayers) == log_h + 1
    for a, b in zip(layers, olayers):
        assert np.array_equal(a, b)
    assert np.array_equal(root, oroot)
    out = p3.mmcs.compress_layer_variant("poseidon2", 1, p3.dev_u32(np.ascontiguousarray(olayers[0])))
    torch.cuda.synchronize()
    assert np.array_equal(p3.host_u32(out), olayers[1])
