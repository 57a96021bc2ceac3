"""CPU tests of the device PCS batch verifier's host half over MIXED heights: p3hip_pcs_proof_len_mixed (it touches no GPU) against the
reference prover of tests/pcs_mixed_ref.py, against the same-height entry, and gate by gate against the host verifier
p3hip_pcs_verify_mixed."""
import ctypes as C

import numpy as np
import pytest

import pcs_many as M
import pcs_many_mixed as MM
import pcs_mixed_ref as MR
import pcs_ref as R

HASHES = M.HASHES


def _len_case(p3, hash, kind, fp, rounds):
    """rounds as pcs_mixed_ref.prove takes them"""
    d = MR.prove(kind, fp, rounds, M.prefix(R.RefChallenger(kind), 3))
    _, slots = M.slots_of([[pts for _, _, pts in mats] for mats in rounds])
    widths = [[m.shape[1] for m, _, _ in mats] for mats in rounds]
    n_slots = 1 + max(s for rs in slots for ms in rs for s in ms)
    got = p3.pcs_proof_len(p3.FriParameters(*fp), hash, d["log_heights"], M.verifier_shape(widths, slots), n_slots)
    assert got == len(d["proof"]), (hash, fp, d["log_heights"], got, len(d["proof"]))
    assert len(MM.word_classes(kind, fp, d["log_heights"], widths)) * 4 == got


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_blowup", [1, 2])
@pytest.mark.parametrize("name", list(MM.SHAPES))
def test_proof_len_equals_the_reference_provers_on_the_mixed_shapes(p3, oracle, hash, kind, log_blowup, name):
    lfp, spec = MM.SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    pts = [R.rand_point(rng) for _ in range(MM.n_slots_of(spec))]
    _len_case(p3, hash, kind, (log_blowup, lfp, 2, 0), MR.mats_of(rng, spec, pts))


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_blowup", [1, 2])
def test_proof_len_equals_the_reference_provers_on_random_mixed_shapes(p3, oracle, hash, kind, log_blowup):
    for seed in range(20):
        rng = np.random.default_rng(300 + seed)
        rounds = MR.random_mixed_case(rng, max_log_h=6, max_cols=200)
        hs = [int(m.shape[0]).bit_length() - 1 for mats in rounds for m, _, _ in mats]
        lfp = int(rng.integers(0, min(min(hs), max(hs) - 1) + 1))
        _len_case(p3, hash, kind, (log_blowup, lfp, int(rng.integers(1, 3)), 0), rounds)


@pytest.mark.parametrize("hash,kind", HASHES)
@pytest.mark.parametrize("log_h", range(1, 8))
def test_equal_heights_give_the_same_height_entrys_length(p3, oracle, hash, kind, log_h):
    rng = np.random.default_rng(400 + 2 * log_h + kind)
    rounds = R.random_case(rng, log_h, max_cols=200)
    _, slots = M.slots_of([[pts for _, _, pts in mats] for mats in rounds])
    widths = [[m.shape[1] for m, _, _ in mats] for mats in rounds]
    n_slots = 1 + max(s for rs in slots for ms in rs for s in ms)
    shape = M.verifier_shape(widths, slots)
    for fp in ((1, 0, 2, 0), (int(rng.integers(1, 3)), int(rng.integers(0, log_h)), int(rng.integers(1, 4)), 3)):
        params = p3.FriParameters(*fp)
        old = p3.pcs_proof_len(params, hash, log_h, shape, n_slots)
        assert p3.pcs_proof_len(params, hash, [[log_h] * len(ws) for ws in widths], shape, n_slots) == old


def test_proof_len_mixed_refuses_what_the_host_verifier_refuses(p3, oracle):
    """each refusal once through p3.pcs.verify with per-matrix heights and once through proof_len: ERR_BAD_ARG and the same message"""
    fp = p3.FriParameters
    ok = fp(1, 0, 2, 0)
    z = R.rand_point(np.random.default_rng(1))
    root = np.zeros(8, dtype=np.uint32)
    # (params, log heights per round, widths per round, points per matrix, what the message says)
    cases = [(ok, [], [], [], "zero rounds"),
             (ok, [[3]] * 5, [[1]] * 5, [[1]] * 5, "5 rounds, at most 4"),
             (ok, [[3], []], [[1], []], [[1], []], "round 1 has zero matrices"),
             (ok, [[3] * 9], [[1] * 9], [[1] * 9], "round 0 has more than 8 matrices"),
             (ok, [[3, 0]], [[2, 2]], [[1, 1]], "LDE height outside"),  # a height below 2^1
             (ok, [[2, 27]], [[2, 2]], [[1, 1]], "LDE height outside"),  # the tallest matrix's LDE
             (fp(0, 0, 2, 0), [[3, 2]], [[2, 2]], [[1, 1]], "LDE height outside"),
             (fp(1, 3, 2, 0), [[3, 2]], [[2, 2]], [[1, 1]], "log_final_poly_len must be below"),
             (fp(1, 0, 2, 31), [[3, 2]], [[2, 2]], [[1, 1]], "proof_of_work_bits"),
             (fp(1, 0, 0, 0), [[3, 2]], [[2, 2]], [[1, 1]], "num_queries"),
             (fp(1, 2, 2, 0), [[4], [3, 1]], [[2], [2, 2]], [[1], [1, 1]], "round 1 matrix 1 has height 2\\^1, below the final polynomial's 2\\^2"),
             (ok, [[4, 2]], [[2, 2]], [[0, 1]], "no matrix of the tallest height 2\\^4 has an opening point"),
             (ok, [[4, 2], [4]], [[2, 2], [3]], [[0, 0], [0]], "no opening point"),
             (ok, [[3, 2]], [[2, 0]], [[1, 1]], "round 0 matrix 1: width must be in"),
             (ok, [[3, 2]], [[8193, 2]], [[1, 1]], "round 0 matrix 0: width must be in"),
             (ok, [[3, 2]], [[2, 2]], [[1, 5]], "round 0 matrix 1: more than 4 opening points"),
             (ok, [[3, 2, 2]], [[4096, 4096, 1]], [[1, 1, 1]], "more than 8192 batched columns"),
             (ok, [[3], [2]], [[2048], [1]], [[4], [1]], "round 1 matrix 0 point 0: more than 8192 batched columns")]
    seen = set()
    for params, lhs, widths, counts, what in cases:
        vr = [((root, ws), [[z] * c for c in cs]) for ws, cs in zip(widths, counts)]
        total = sum(w * c for ws, cs in zip(widths, counts) for w, c in zip(ws, cs))
        with pytest.raises(p3.P3HipError, match=what) as host:
            p3.pcs.verify(params, "poseidon2", vr, lhs, np.zeros((total, 4), np.uint32), b"\0" * 8, p3.Challenger("poseidon2"))
        assert host.value.code == M.BAD_ARG
        shape = [[(w, [0] * c) for w, c in zip(ws, cs)] for ws, cs in zip(widths, counts)]
        with pytest.raises(p3.P3HipError) as mine:
            p3.pcs_proof_len(params, "poseidon2", lhs, shape, 1)
        assert mine.value.code == M.BAD_ARG and mine.value.message == host.value.message, (mine.value.message, host.value.message)
        seen.add(mine.value.message)
    assert len(seen) >= 16, sorted(seen)  # the cases name different gates
    # the slots are the batch verifier's own
    for n_slots, slot, what in ((0, 0, "n_slots"), (5, 0, "n_slots"), (2, 2, "slot 2 of 2")):
        with pytest.raises(p3.P3HipError, match=what) as e:
            p3.pcs_proof_len(ok, "poseidon2", [[3, 2]], [[(2, [slot]), (1, [])]], n_slots)
        assert e.value.code == M.BAD_ARG


def test_hiding_is_refused_with_per_matrix_heights(p3, oracle):
    ok = p3.FriParameters(1, 0, 2, 0)
    shape = [[(2, [0]), (3, [0])]]
    with pytest.raises(ValueError, match="a hiding PCS takes one log height"):
        p3.pcs_proof_len(ok, "poseidon2", [[3, 2]], shape, 1, hiding=True)
    with pytest.raises(ValueError, match="one log height per matrix"):
        p3.pcs_proof_len(ok, "poseidon2", [[3]], shape, 1)
    # lists and tuples are per-matrix heights; anything else goes down the same-height path
    assert p3.pcs_proof_len(ok, "poseidon2", ((3, 2),), shape, 1) == p3.pcs_proof_len(ok, "poseidon2", [[3, 2]], shape, 1)
    assert p3.pcs_proof_len(ok, "poseidon2", np.int64(3), shape, 1) == p3.pcs_proof_len(ok, "poseidon2", 3, shape, 1)
    with pytest.raises(TypeError):
        p3.pcs_proof_len(ok, "poseidon2", None, shape, 1)
    # the C entry takes the flag, so that a hiding PCS over mixed heights needs no new one; today it refuses it by name
    lib = p3._lib.lib()
    sh, _keep = p3.pcs._shape(0, shape, 1)
    lhs, out = (C.c_uint * 2)(3, 2), C.c_size_t()
    args = (C.cast(ok._c(), C.c_void_p), C.byref(sh))
    assert lib.p3hip_pcs_proof_len_mixed(0, 1, *args, lhs, C.byref(out)) == M.BAD_ARG
    msg = p3._lib.take_last_error()
    assert "mixed heights" in msg and "HidingFriPcs" in msg, msg
    assert lib.p3hip_pcs_proof_len_mixed(0, 0, *args, None, C.byref(out)) == M.BAD_ARG
    assert "null argument" in p3._lib.take_last_error()
    assert lib.p3hip_pcs_proof_len_mixed(0, 0, *args, lhs, C.byref(out)) == 0 and out.value == p3.pcs_proof_len(ok, "poseidon2", [[3, 2]], shape, 1)
