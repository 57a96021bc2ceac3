"""GPU tests of the device TwoAdicFriPcs over matrices of MIXED heights (TwoAdicFriPcs(mixed_heights=True): csrc/pcs.hip.inc,
fri_fold_rollin_kernel of csrc/prover.hip) against the reference prover of tests/pcs_mixed_ref.py: roots, opened values, FriProof
bytes and the next transcript sample are compared, and both host verifiers accept.  The shapes are the smallest at which each new
branch can go wrong; one is past the tree code's small-layer thresholds."""
import gc

import numpy as np
import pytest

import pcs_mixed_ref as M
import pcs_ref as R

pytestmark = pytest.mark.gpu
P = R.P
PREFIX = np.arange(1, 6, dtype=np.uint32)  # some transcript before the open
KIND = {"poseidon2": 0, "keccak": 1}


def _device(p3, pcs, hash, rounds):
    datas = [pcs.commit([(m, s) for m, s, _ in mats]) for mats in rounds]
    ch = p3.Challenger(hash)
    ch.observe(PREFIX)
    opened, fri = pcs.open([(d, [pts for _, _, pts in mats]) for (_, d), mats in zip(datas, rounds)], ch)
    for _, d in datas:
        d.free()
    return [r for r, _ in datas], opened, fri, ch


def _compare(p3, hash, profile, t, rounds, pcs=None, ref=None):
    """device open == reference prover; with queries, both host verifiers accept and stand where the prover stands"""
    kind = KIND[hash]
    own = pcs is None
    if own:
        pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, profile, mixed_heights=True)
    roots, opened, fri, ch = _device(p3, pcs, hash, rounds)
    if own:
        pcs.free()
    if ref is None:
        pch = R.RefChallenger(kind)
        pch.observe(PREFIX)
        ref = (M.prove(kind, t, rounds, pch), pch.sample_ext())
    d, want = ref
    for r, (a, b) in enumerate(zip(roots, d["roots"])):
        assert np.array_equal(a, b), "root of round %d" % r
    assert opened.shape == d["opened"].shape
    if not np.array_equal(opened, d["opened"]):
        pytest.fail("opened values differ first at %d of %d" % (int(np.nonzero((opened != d["opened"]).any(axis=1))[0][0]), len(opened)))
    assert len(fri) == len(d["proof"]), (len(fri), len(d["proof"]))
    if fri != d["proof"]:
        w1, w2 = np.frombuffer(fri, np.uint32), np.frombuffer(d["proof"], np.uint32)
        pytest.fail("FriProof words differ first at %d of %d" % (int(np.nonzero(w1 != w2)[0][0]), len(w1)))
    assert np.array_equal(ch.sample_ext(), want)
    if t[2]:
        vr, lhs = M.verifier_rounds(roots, rounds)
        c = p3.Challenger(hash)
        c.observe(PREFIX)
        p3.pcs.verify(p3.FriParameters(*t), hash, vr, lhs, opened, fri, c)  # accepts
        assert np.array_equal(c.sample_ext(), want)
        rc = R.RefChallenger(kind)
        rc.observe(PREFIX)
        assert M.verify(kind, t, lhs, vr, opened, fri, rc) == 0
    return ref


# name -> (log_final_poly_len, [[(log_h, width, [point index]) per matrix] per round])
SHAPES = {
    # a roll-in at the very first fold, the smallest possible
    "first fold": (0, [[(2, 3, [0]), (1, 2, [0, 1])]]),
    # roll-ins at consecutive folds; a round whose tree is shorter than the index
    "consecutive folds": (0, [[(3, 2, [0, 1]), (1, 5, [1])], [(2, 3, [0])]]),
    # a roll-in into the final vector; one class over two rounds: its alpha counter carries across rounds
    "final vector": (1, [[(4, 3, [0]), (1, 2, [0, 1])], [(3, 5, [1]), (4, 2, [1, 0])]]),
    # folds without a roll-in between classes; a commitment in non-monotone height order
    "gap": (2, [[(5, 2, [0]), (2, 3, [1]), (3, 7, [0, 1])]]),
    # a width-17 matrix of a small class: the tile kernel with fewer than 64 rows, the barycentric kernel with h below its block
    "wide small class": (0, [[(4, 3, [0]), (2, 17, [0, 1]), (4, 2, [1]), (1, 5, [0])]]),
    # a small-class matrix without points next to one of that class with points
    "no points beside points": (0, [[(4, 3, [0]), (2, 5, []), (2, 4, [0, 1])]]),
    # a class whose every matrix has no points: no vector and no roll-in at that height, the openings are still served
    "class without points": (0, [[(4, 3, [0, 1]), (2, 5, []), (2, 2, [])], [(3, 2, [1]), (2, 19, [])]]),
    # four points on a small-class matrix; a point shared between classes: one range of the d table's row per class
    "four points": (0, [[(4, 2, [0]), (2, 3, [0, 1, 2, 3])]]),
}
# (hash, profile, log_blowup, num_queries, pow_bits): both hashes and profiles, queries 0 and 5, bits 0 and 4, blowup 1 and 2
CONFIGS = [("poseidon2", "latency", 1, 5, 4), ("keccak", "throughput", 2, 5, 0), ("poseidon2", "throughput", 2, 0, 4), ("keccak", "latency", 1, 0, 0),
           ("keccak", "latency", 2, 5, 4), ("poseidon2", "throughput", 1, 5, 0)]


def _cases():
    out = []
    for i, name in enumerate(SHAPES):
        for j in (0, 1, 2):  # three of the six configurations per shape, rotating: every shape sees both hashes and a run with queries
            out.append((name, CONFIGS[(i + 2 * j) % 6]))
    return out


for _k, _vals in enumerate([{"poseidon2", "keccak"}, {"latency", "throughput"}, {1, 2}, {0, 5}, {0, 4}]):
    assert {c[1][_k] for c in _cases()} == _vals
for _name in SHAPES:
    _mine = [c[1] for c in _cases() if c[0] == _name]
    assert {m[0] for m in _mine} == {"poseidon2", "keccak"} and any(m[3] for m in _mine)


@pytest.mark.parametrize("name,config", _cases(), ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_device_open_equals_the_reference_prover(p3, oracle, name, config):
    hash, profile, log_blowup, nq, bits = config
    lfp, spec = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    pts = [R.rand_point(rng) for _ in range(3)] + [R.ext_from_base(R.ONE)]  # the last one in the base field, off every coset
    _compare(p3, hash, profile, (log_blowup, lfp, nq, bits), M.mats_of(rng, spec, pts))


@pytest.mark.parametrize("hash,profile", [("poseidon2", "latency"), ("keccak", "throughput")])
def test_a_shape_past_the_small_layer_thresholds(p3, oracle, hash, profile):
    """log_h 13, 10 and 5, widths 4, 20 and 64: trees, folds and roll-ins that take the bulk kernels"""
    rng = np.random.default_rng(13)
    pts = [R.rand_point(rng), R.rand_point(rng)]
    rounds = M.mats_of(rng, [[(13, 4, [0, 1]), (10, 20, [0])], [(5, 64, [1]), (10, 3, [1])]], pts)
    _compare(p3, hash, profile, (1, 1, 5, 4), rounds)


def test_ten_opens_alternate_mixed_and_same_height_shapes(p3, oracle):
    """one object, the arena rebuilt at every change of shape and reused between two opens of one shape; a same-height open on a
    mixed-enabled object is pcs_ref.open; no device memory is lost"""
    import torch
    t, hash, kind = (1, 1, 5, 2), "poseidon2", 0
    rng = np.random.default_rng(10)
    pts = [R.rand_point(rng), R.rand_point(rng)]
    # the shorter class has 2^16 LDE rows: its reduced-opening vector, the one allocation a mixed arena adds, takes 1 MiB, so a
    # rebuild that loses it alone shows; the whole mixed arena is above 8 MiB
    mixed = M.mats_of(rng, [[(16, 2, [0]), (15, 3, [0, 1])], [(15, 2, [1])]], pts)
    same = M.mats_of(rng, [[(11, 3, [0]), (11, 17, [0, 1])], [(11, 5, [1])]], pts)
    pch = R.RefChallenger(kind)
    pch.observe(PREFIX)
    o, f = R.open(kind, t, 11, same, pch)
    same_ref = ({"opened": o, "proof": f, "roots": [R.commit(kind, t[0], [(m, s) for m, s, _ in mats])[0] for mats in same]}, pch.sample_ext())
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash, mixed_heights=True)

    def free_bytes():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()  # the uploads of the test's own matrices go through torch's caching allocator: not the library's memory
        return torch.cuda.mem_get_info()[0]

    oracle.set_threads(oracle.test_threads())  # the reference's trees over 2^17 rows
    try:
        pch = R.RefChallenger(kind)
        pch.observe(PREFIX)
        mixed_ref = (M.prove(kind, t, mixed, pch), pch.sample_ext())
    finally:
        oracle.set_threads(1)
    _compare(p3, hash, "latency", t, same, pcs, same_ref)
    _compare(p3, hash, "latency", t, mixed, pcs, mixed_ref)
    base = free_bytes()  # the mixed shape's arena is live here and again after the last open
    for k in range(10):  # mixed, mixed, same, same, mixed, ...: every second open finds its arena, two of the rebuilds are mixed
        if (k // 2) % 2 == 0:
            _compare(p3, hash, "latency", t, mixed, pcs, mixed_ref)
        else:
            _compare(p3, hash, "latency", t, same, pcs, same_ref)
    lost = base - free_bytes()
    pcs.free()
    # a rebuild that lost anything of a mixed arena lost at least the 1 MiB of the shorter class's vector
    assert lost < (1 << 20), "free device memory fell by %d bytes over ten opens" % lost


def test_default_and_hiding_objects_still_refuse_mixed_heights(p3, oracle):
    rng = np.random.default_rng(3)
    m8, m16 = R.rand_matrix(rng, 3, 3), R.rand_matrix(rng, 4, 3)
    z = R.rand_point(rng)
    mixed = p3.TwoAdicFriPcs(p3.FriParameters(1, 0, 2, 1), mixed_heights=True)
    _, dm = mixed.commit([(m8, None), (m16, None)])
    for pcs in (p3.TwoAdicFriPcs(p3.FriParameters(1, 0, 2, 1)), p3.HidingFriPcs(p3.FriParameters(1, 0, 2, 1))):
        with pytest.raises(p3.P3HipError, match="matrix 1 has height 16, matrix 0 has 8: mixed heights are not supported"):
            pcs.commit([(m8, None), (m16, None)])
        pcs.free()
    plain = p3.TwoAdicFriPcs(p3.FriParameters(1, 0, 2, 1))
    (_, d8), (_, d16) = plain.commit([(m8, None)]), plain.commit([(m16, None)])
    ch = p3.Challenger()
    with pytest.raises(p3.P3HipError, match="round 1 matrix 0 has height 2\\^4, round 0 has 2\\^3: mixed heights are not supported"):
        plain.open([(d8, [[z]]), (d16, [[z]])], ch)
    # prover data of a mixed commitment, handed to an object that was not created for it
    with pytest.raises(p3.P3HipError, match="round 0 matrix 0 has height 2\\^3, round 0 has 2\\^4: mixed heights are not supported"):
        plain.open([(dm, [[z], [z]])], ch)
    assert np.array_equal(ch.sample_ext(), p3.Challenger().sample_ext())
    # what the plain object committed serves a mixed open: heights are per matrix
    opened, _ = mixed.open([(d8, [[z]]), (d16, [[z]])], p3.Challenger())
    assert np.array_equal(opened[:3], R.opened_value(m8, R.ONE, z)) and np.array_equal(opened[3:], R.opened_value(m16, R.ONE, z))
    assert tuple(mixed.get_evaluations_on_domain(dm, 0, 4).shape) == (16, 3) and tuple(mixed.get_evaluations_on_domain(dm, 1, 5).shape) == (32, 3)
    with pytest.raises(ValueError, match="between the matrix height and the LDE height"):
        mixed.get_evaluations_on_domain(dm, 0, 5)


def test_the_mixed_object_refuses_by_name_and_leaves_the_challenger(p3, oracle):
    rng = np.random.default_rng(4)
    m2, m8, m16 = R.rand_matrix(rng, 1, 2), R.rand_matrix(rng, 3, 3), R.rand_matrix(rng, 4, 3)
    z = R.rand_point(rng)
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(1, 0, 2, 1), mixed_heights=True)
    _, d = pcs.commit([(m8, None), (m16, None), (m2, None)])
    ch = p3.Challenger()
    with pytest.raises(p3.P3HipError, match="no matrix of the tallest height 2\\^4 has an opening point: the FRI input would be missing"):
        pcs.open([(d, [[z], [], [z]])], ch)
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(5), 3)))  # on GENERATOR <g_32>, not on GENERATOR <g_16> or <g_4>
    assert R.bpow(R.bmul(int(on[0]), R.binv(R.GEN)), 16) != R.ONE
    with pytest.raises(p3.P3HipError, match="round 0 matrix 2 point 1 lies on the LDE coset"):
        pcs.open([(d, [[z], [z], [z, on]])], ch)
    with pytest.raises(p3.P3HipError, match="9 matrices, a commitment holds at most 8"):
        pcs.commit([(m8, None)] * 8 + [(m2, None)])
    with pytest.raises(p3.P3HipError, match="matrix 1: height must be a power of two >= 2"):
        pcs.commit([(m8, None), (m2[:1], None)])
    with pytest.raises(p3.P3HipError, match="5 rounds, an open takes at most 4"):
        pcs.open([(d, [[z], [z], [z]])] * 5, ch)
    with pytest.raises(p3.P3HipError, match="more than 4 distinct opening points"):
        pcs.open([(d, [[R.ext_from_base(int(R.O.to_monty(k))) for k in range(2, 5)], [z], [R.ext_from_base(R.ONE)]])], ch)
    low = p3.TwoAdicFriPcs(p3.FriParameters(1, 2, 2, 1), mixed_heights=True)
    _, dl = low.commit([(m16, None), (m2, None)])
    with pytest.raises(p3.P3HipError, match="round 0 matrix 1 has height 2\\^1, below the final polynomial's 2\\^2"):
        low.open([(dl, [[z], [z]])], ch)
    with pytest.raises(p3.P3HipError, match="LDE domain above 2\\^26"):
        p3.TwoAdicFriPcs(p3.FriParameters(24, 0, 2, 1), mixed_heights=True).commit([(m2, None), (m8, None)])
    assert np.array_equal(ch.sample_ext(), p3.Challenger().sample_ext())  # none of the refused calls moved the transcript
    opened, fri = pcs.open([(d, [[z], [z], []])], p3.Challenger())  # and the object still works
    assert np.array_equal(opened[:3], R.opened_value(m8, R.ONE, z))
