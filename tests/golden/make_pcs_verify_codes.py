#!/usr/bin/env python3
"""What the PCS host verifiers (p3hip_pcs_verify / _mixed / _hiding) and p3hip_pcs_proof_len[_mixed] answer, recorded so that a later
build can be held against an earlier one:   python3 tests/golden/make_pcs_verify_codes.py   ->   tests/golden/pcs_verify_codes.json

  refusals   every refused-argument case of test_proof_len_refuses_what_the_host_verifiers_refuse, its mixed twin,
             test_argument_gates_name_the_offender, test_refusals_by_message and test_hiding_verify_argument_gates (their tables
             restated: they are local to the tests): [code, message] of the host verifier, and of pcs_proof_len over the same shape
             (slots from the distinct points; [0, length] where it takes the shape)
  lens       pcs_proof_len on the shapes of test_proof_len_equals_the_reference_provers_plain / _hiding (the same seeds), on every
             shape of pcs_many_mixed.SHAPES at log_blowup 1 and 2, and on DEEP
  tampered   the host verifier's code after tampering each word of a proof in turn (pcs_many.tampered), one code per word: shape A and
             shape B of tests/pcs_many.py and pcs_many_mixed.EVERY_WORD, under both hashes
  two_faults the host verifier's CODE (the message may name either fault) where a shape fault follows a non-canonical or on-coset point
             in round -> matrix -> point order
The proofs come from the reference provers of tests/ with seeded generators.  tests/test_pcs_layout_parent_host.py recomputes record()
on the current build."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

import pcs_hiding_ref as H  # noqa: E402
import pcs_many as M  # noqa: E402
import pcs_many_mixed as MM  # noqa: E402
import pcs_mixed_ref as MR  # noqa: E402
import pcs_ref as R  # noqa: E402

OUT = os.path.join(HERE, "pcs_verify_codes.json")
ROOT8 = np.zeros(8, dtype=np.uint32)


def _answer(p3, fn):
    try:
        r = fn()
    except p3.PcsRejected as e:
        return [int(e.code), ""]
    except p3.P3HipError as e:
        return [int(e.code), e.message]
    return [0, 0 if r is None else int(r)]


def _zeros(vr):
    return np.zeros((sum(int(w) * len(pts) for (_, ws), mp in vr for w, pts in zip(ws, mp)), 4), np.uint32)


def _both(p3, params, vr, log_h, hiding=False, opened=None, proof=b"\0" * 8, ch=None, hash="poseidon2"):
    """the host verifier and pcs_proof_len on one set of arguments; vr as p3.pcs.verify takes it"""
    params = p3.FriParameters(*params)
    ch = ch.clone() if ch is not None else p3.Challenger("poseidon2")
    host = _answer(p3, lambda: p3.pcs.verify(params, hash, vr, log_h, _zeros(vr) if opened is None else opened, proof, ch, hiding=hiding))
    mat_points = [mp for _, mp in vr]
    if any(len(pts) for mp in mat_points for pts in mp):
        pool, slots = M.slots_of(mat_points)
    else:
        pool, slots = [None], [[[] for _ in mp] for mp in mat_points]
    shape = M.verifier_shape([ws for (_, ws), _ in vr], slots)
    return {"host": host, "len": _answer(p3, lambda: p3.pcs_proof_len(params, hash, log_h, shape, len(pool), hiding=hiding))}


def _vr(widths, counts, z):
    return [((ROOT8, ws), [[z] * c for c in cs]) for ws, cs in zip(widths, counts)]


def refusals(p3, oracle):
    from test_pcs_verify_host import _instance, _prefix, _rounds
    out = []
    ok = (1, 0, 2, 0)
    z = R.rand_point(np.random.default_rng(1))
    # test_proof_len_refuses_what_the_host_verifiers_refuse: (params, log_h, widths per round, points per matrix, hiding)
    for params, log_h, widths, counts, hiding in [
            ((0, 0, 2, 0), 3, [[2]], [[1]], False), ((1, 3, 2, 0), 3, [[2]], [[1]], False), ((1, 0, 2, 31), 3, [[2]], [[1]], False),
            ((1, 0, 0, 0), 3, [[2]], [[1]], False), (ok, 27, [[2]], [[1]], False), (ok, 3, [], [], False),
            (ok, 3, [[1]] * 5, [[1]] * 5, False), (ok, 3, [[]], [[]], False), (ok, 3, [[1] * 9], [[1] * 9], False),
            (ok, 3, [[1] * 5], [[1] * 5], True), (ok, 3, [[0]], [[1]], False), (ok, 3, [[8193]], [[1]], False),
            (ok, 3, [[2]], [[5]], False), (ok, 3, [[4096, 4096, 1]], [[1, 1, 1]], False), (ok, 3, [[2049]], [[4]], False),
            (ok, 3, [[2], [3]], [[0], [0]], False), (ok, 27, [[2]], [[1]], True), ((1, 3, 2, 0), 2, [[2]], [[1]], True),
            (ok, 0, [[2]], [[1]], True)]:
        out.append(_both(p3, params, _vr(widths, counts, z), log_h, hiding))
    # test_proof_len_mixed_refuses_what_the_host_verifier_refuses: (params, log heights, widths, points per matrix)
    for params, lhs, widths, counts in [
            (ok, [], [], []), (ok, [[3]] * 5, [[1]] * 5, [[1]] * 5), (ok, [[3], []], [[1], []], [[1], []]),
            (ok, [[3] * 9], [[1] * 9], [[1] * 9]), (ok, [[3, 0]], [[2, 2]], [[1, 1]]), (ok, [[2, 27]], [[2, 2]], [[1, 1]]),
            ((0, 0, 2, 0), [[3, 2]], [[2, 2]], [[1, 1]]), ((1, 3, 2, 0), [[3, 2]], [[2, 2]], [[1, 1]]),
            ((1, 0, 2, 31), [[3, 2]], [[2, 2]], [[1, 1]]), ((1, 0, 0, 0), [[3, 2]], [[2, 2]], [[1, 1]]),
            ((1, 2, 2, 0), [[4], [3, 1]], [[2], [2, 2]], [[1], [1, 1]]), (ok, [[4, 2]], [[2, 2]], [[0, 1]]),
            (ok, [[4, 2], [4]], [[2, 2], [3]], [[0, 0], [0]]), (ok, [[3, 2]], [[2, 0]], [[1, 1]]), (ok, [[3, 2]], [[8193, 2]], [[1, 1]]),
            (ok, [[3, 2]], [[2, 2]], [[1, 5]]), (ok, [[3, 2, 2]], [[4096, 4096, 1]], [[1, 1, 1]]),
            (ok, [[3], [2]], [[2048], [1]], [[4], [1]])]:
        out.append(_both(p3, params, _vr(widths, counts, z), lhs))
    # test_argument_gates_name_the_offender: the oracle's fib proof at log_n = 3, one argument wrong at a time
    t, log_n = (1, 0, 3, 2), 3
    pis, _, root_t, root_q, opened, fri = _instance(oracle, 0, log_n, t)
    ch, zeta, zeta_next = _prefix(p3, "poseidon2", log_n, pis, root_t, root_q)
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_n + 1), 5)))
    pts = [R.ext_from_base(int(oracle.to_monty(k))) for k in range(2, 7)]
    bad = opened.copy()
    bad[3, 1] = R.P
    rounds = _rounds(root_t, root_q, zeta, zeta_next)
    for vr, kw in [
            (_rounds(root_t, root_q, zeta, on), {}), ([((root_t, [2]), [[zeta, zeta_next]]), ((root_q, [4]), [[on]])], {}),
            ([((root_t, [2]), [[zeta, zeta_next]]), ((root_q, []), [])], dict(opened=opened[:4])), ([], dict(opened=None)),
            ([((root_t, [2]), [[]])], dict(opened=None)), ([((root_t, [1] * 9), [[zeta]] * 9)], dict(opened=None)),
            ([((root_t, [1]), [[zeta]])] * 5, dict(opened=None)), ([((root_t, [1]), [pts])], dict(opened=None)),
            ([((root_t, [1]), [pts[:4]]), ((root_q, [1]), [pts[4:]])], dict(opened=None)),
            ([((root_t, [8000, 193]), [[zeta], [zeta]])], dict(opened=None)), ([((root_t, [0]), [[zeta]])], dict(opened=None)),
            (_rounds(root_t, root_q, np.array([R.P, 0, 0, 0], np.uint32), zeta_next), {}), (rounds, dict(opened=bad)),
            (rounds, dict(params=(1, 3, 3, 2))), (rounds, dict(params=(1, 0, 0, 2))), (rounds, dict(params=(1, 0, 3, 31))),
            (rounds, dict(params=(0, 0, 3, 2))), (rounds, dict(log_h=0)), (rounds, dict(hash="keccak"))]:
        kw = dict(dict(opened=opened, params=t, log_h=log_n, hash="poseidon2"), **kw)
        out.append(_both(p3, kw["params"], vr, kw["log_h"], opened=kw["opened"], proof=fri, ch=ch, hash=kw["hash"]))
    # test_refusals_by_message (mixed heights)
    z = R.rand_point(np.random.default_rng(11))
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(4), 3)))
    for params, lhs, vr in [
            (ok, [[3, 2]], [((ROOT8, [2, 2]), [[], [z]])]), ((1, 2, 2, 0), [[4], [1]], [((ROOT8, [2]), [[z]]), ((ROOT8, [3]), [[z]])]),
            (ok, [[3, 1]], [((ROOT8, [2, 2]), [[z], [z, on]])]), (ok, [[3, 1]] * 5, [((ROOT8, [2, 2]), [[z], [z]])] * 5),
            (ok, [[3] * 9], [((ROOT8, [1] * 9), [[z]] * 9)]), (ok, [[3, 0]], [((ROOT8, [2, 2]), [[z], [z]])]),
            ((2, 0, 2, 0), [[26, 3]], [((ROOT8, [2, 2]), [[z], [z]])]), ((1, 3, 2, 0), [[3, 3]], [((ROOT8, [2, 2]), [[z], [z]])]),
            (ok, [[3, 1]], [((ROOT8, [2, 2]), [pts[:3], pts[3:]])]), (ok, [[3, 1]], [((ROOT8, [8000, 200]), [[z], [z]])])]:
        out.append(_both(p3, params, vr, lhs, proof=b"\0" * 64))
    # test_hiding_verify_argument_gates
    t, log_h = (1, 0, 10, 1), 2
    pcs = H.HidingPcs(0, t, 3)
    rng = np.random.default_rng(9)
    z = R.rand_point(rng)
    com = pcs.commit([(R.rand_matrix(rng, log_h, 2), None)])
    opened, fri = pcs.open([(com, [[z]])], R.RefChallenger(0))
    vr = [((com.root, [5]), [[z]])]
    on = R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_h + 2), 3)))
    for v, kw in [([((com.root, [1] * 5), [[z]] * 5)], dict(opened=None)), (vr, dict(params=(1, 3, 10, 1))), (vr, dict(log_h=0)),
                  ([((com.root, [5]), [[on]])], {})]:
        kw = dict(dict(opened=opened, params=t, log_h=log_h), **kw)
        out.append(_both(p3, kw["params"], v, kw["log_h"], True, opened=kw["opened"], proof=fri))
    for c in out:
        assert c["host"][0] == M.BAD_ARG, c
    return out


def lens(p3, oracle):
    out = {}
    for hash, kind in M.HASHES:
        for log_h in range(1, 8):
            rng = np.random.default_rng(100 + 2 * log_h + kind)  # test_proof_len_equals_the_reference_provers_plain
            fp = (int(rng.integers(1, 3)), int(rng.integers(0, log_h)), int(rng.integers(1, 4)), int(rng.integers(0, 3)))
            for name, rounds, f in (("random", R.random_case(rng, log_h, max_cols=200), fp), ("empty", R.empty_point_case(rng, log_h), (1, 0, 2, 0))):
                pool, slots = M.slots_of([[pts for _, _, pts in mats] for mats in rounds])
                shape = M.verifier_shape([[m.shape[1] for m, _, _ in mats] for mats in rounds], slots)
                out["plain %s %s %d" % (name, hash, log_h)] = p3.pcs_proof_len(p3.FriParameters(*f), hash, log_h, shape, len(pool))
            rng = np.random.default_rng(200 + 2 * log_h + kind)  # ..._hiding
            fp = (int(rng.integers(1, 3)), int(rng.integers(0, log_h + 1)), int(rng.integers(1, 4)), int(rng.integers(0, 3)))
            pcs = H.HidingPcs(kind, fp, (1, 3, 4)[log_h % 3], mmcs_seed=log_h, pcs_seed=7 + kind)
            _, rounds = H.random_rounds(rng, pcs, log_h, (1, 2, 17), max_rounds=3, max_mats=3, randomization=log_h % 2 == 1, max_cols=200)
            if len(rounds) > 1 and any(p for _, mp in rounds[1:] for p in mp):
                rounds[0] = (rounds[0][0], [[] for _ in rounds[0][1]])
            pool, slots = M.slots_of([mp for _, mp in rounds])
            shape = M.verifier_shape([com.widths for com, _ in rounds], slots)
            out["hiding %s %d" % (hash, log_h)] = p3.pcs_proof_len(p3.FriParameters(*fp), hash, log_h, shape, len(pool), hiding=True)
        for name, (lfp, spec) in list(MM.SHAPES.items()) + [("DEEP", MM.DEEP)]:
            for fp in [MM.DEEP[0]] if name == "DEEP" else [(1, lfp, 2, 0), (2, lfp, 2, 0)]:
                out["mixed %s %s %d" % (name, hash, fp[0])] = p3.pcs_proof_len(p3.FriParameters(*fp), hash, MM.heights_of(spec), MM.verifier_shape(spec),
                                                                               MM.n_slots_of(spec))
    return {k: int(v) for k, v in out.items()}


def _word_by_word(p3, fp, hash, hiding, log_h, widths, roots, mat_points, opened, proof, state):
    assert M.host_code(p3, fp, hash, hiding, log_h, widths, roots, mat_points, opened, proof, state)[0] == 0
    words, codes = np.frombuffer(proof, dtype=np.uint32), []
    for i in range(len(words)):
        t = words.copy()
        t[i] = M.tampered(t[i])
        codes.append(int(M.host_code(p3, fp, hash, hiding, log_h, widths, roots, mat_points, opened, t.tobytes(), state)[0]))
    return codes


def tampered(p3, oracle):
    out = {}
    for hash, kind in M.HASHES:
        for hiding in (False, True):  # shapes A and B, built as test_pcs_verify_many_host._share builds them
            rng = np.random.default_rng(900 + kind + 2 * hiding)
            fp, log_h = M.FP_AB, M.LOG_H_AB
            pts = np.stack([R.rand_point(rng) for _ in range(2)])
            mat_points = M.expand(pts, M.SLOTS_AB)
            evals = [[(R.rand_matrix(rng, log_h, w), R.rand_shift(rng)) for w in ws] for ws in M.WIDTHS_AB]
            ref = M.prefix(R.RefChallenger(kind), 5)
            if hiding:
                pcs = H.HidingPcs(kind, fp, M.NRC_B, 3, 4)
                rounds = [(pcs.commit(mats), mp) for mats, mp in zip(evals, mat_points)]
                opened, proof = pcs.open(rounds, ref)
                roots, widths = [com.root for com, _ in rounds], [com.widths for com, _ in rounds]
            else:
                rounds = [[(m, s, mp) for (m, s), mp in zip(mats, mps)] for mats, mps in zip(evals, mat_points)]
                opened, proof, roots = R.open_with_roots(kind, fp, log_h, rounds, ref)
                widths = M.WIDTHS_AB
            state = M.prefix(p3.Challenger(hash), 5).export_state()
            out["%s %s" % ("B" if hiding else "A", hash)] = _word_by_word(p3, fp, hash, hiding, log_h, widths, roots, mat_points, opened, proof, state)
        fp, spec = MM.EVERY_WORD
        rng = np.random.default_rng(77 + kind)
        pts = np.stack([R.rand_point(rng) for _ in range(MM.n_slots_of(spec))])
        d = MR.prove(kind, fp, MR.mats_of(rng, spec, pts), M.prefix(R.RefChallenger(kind), 4))
        state = M.prefix(p3.Challenger(hash), 4).export_state()
        out["EVERY_WORD %s" % hash] = _word_by_word(p3, fp, hash, False, d["log_heights"], MM.widths_of(spec), d["roots"], M.expand(pts, MM.slots_of(spec)),
                                                    d["opened"], d["proof"], state)
    return out


def two_faults(p3, oracle):
    ok = (1, 0, 2, 0)
    z = R.rand_point(np.random.default_rng(3))
    nc = np.array([1, R.P, 0, 0], np.uint32)  # no field element
    on = lambda log_big: R.ext_from_base(R.bmul(R.GEN, R.bpow(R.two_adic_generator(log_big), 3)))  # on GENERATOR <g_big>
    cases = [  # (params, log_h or log heights, rounds, hiding): the point's fault comes first in round -> matrix -> point order
        (ok, 3, [((ROOT8, [2]), [[nc]]), ((ROOT8, []), [])], False),                      # ... round 1 has zero matrices
        (ok, 3, [((ROOT8, [2]), [[z, on(4)]]), ((ROOT8, [0]), [[z]])], False),            # ... round 1 matrix 0: width
        (ok, 3, [((ROOT8, [2, 1]), [[nc], [z] * 5])], False),                             # ... more than 4 opening points
        (ok, 3, [((ROOT8, [8000, 193]), [[on(4)], [z]])], False),                         # ... more than 8192 batched columns
        ((1, 2, 2, 0), [[4], [1]], [((ROOT8, [2]), [[nc]]), ((ROOT8, [3]), [[z]])], False),  # ... below the final polynomial's height
        (ok, [[2, 3]], [((ROOT8, [2, 2]), [[on(4)], []])], False),                        # ... no matrix of the tallest height has a point
        (ok, 3, [((ROOT8, [5]), [[on(5)]]), ((ROOT8, [1] * 5), [[z]] * 5)], True),        # ... round 1 has more than 4 matrices
    ]
    out = []
    for params, log_h, vr, hiding in cases:
        code = _both(p3, params, vr, log_h, hiding)["host"][0]
        assert code == M.BAD_ARG
        out.append(code)
    return out


SECTIONS = {"refusals": refusals, "lens": lens, "tampered": tampered, "two_faults": two_faults}


def record(p3, oracle, section):
    return json.loads(json.dumps(SECTIONS[section](p3, oracle)))


if __name__ == "__main__":
    from conftest import load_package
    from oracle import oracle as o
    o.build()
    p3 = load_package()
    with open(OUT, "w") as f:
        json.dump({s: record(p3, o, s) for s in SECTIONS}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
