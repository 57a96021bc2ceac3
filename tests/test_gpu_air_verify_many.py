"""GPU tests of the device batch verifier of caller-defined AIRs (include/p3hip.h p3hip_air_verifier_*; csrc/air_verifier_dev.hip).
Proofs come from the reference prover of tests/air_ref.py (CPU) and from prove_air (device); the expected status of every member
comes from the host verifier p3hip_air_verify through the contract of tests/air_many.py.  No test provokes a fault: what the library
refuses never reaches a launch."""
import gc

import numpy as np
import pytest

import air_many as AM
import air_ref as A
import dev_buffers as DB
import pcs_many as M

pytestmark = pytest.mark.gpu
P = AM.P
FRI = {"fib": (1, 0, 4, 2), "B": (2, 1, 4, 2), "C": (2, 0, 3, 1), "D": (3, 0, 3, 1)}
INSTANCES = {"fib": [dict(a=0, b=1), dict(a=7, b=11), dict(a=P - 1, b=1), dict(a=3, b=4)],
             "B": [dict(), dict(x0=9, y0=2, z0=7), dict(x0=P - 1, y0=1, z0=0), dict(x0=1, y0=0, z0=P - 1)],
             "C": [dict(), dict(s=12345), dict(s=P - 2), dict(s=0)],
             "D": [dict(), dict(s=8, y0=1), dict(s=P - 1, y0=P - 1), dict(s=0, y0=0)]}


@pytest.fixture(scope="module")
def airs(p3, oracle):
    return A.all_airs(p3)


def gpu_proof(p3, air, trace, pis, hash, t):
    pcs = p3.TwoAdicFriPcs(p3.FriParameters(*t), hash)
    proof = p3.prove_air(air, pcs, p3.dev_u32(trace), pis)
    pcs.free()
    return proof


def dev_entry(p3, v, proofs, pis, with_lens=True, pad=0, count=True):
    """-> (statuses, rejected count or None) through p3hip_air_verifier_verify_dev.  The proofs buffer is exactly as large as the
    stride requires; d_status and d_rejected sit between guard words, 4-byte aligned and no more."""
    import torch
    n, stride = len(proofs), v.proof_len + pad
    buf = np.zeros(max(n * stride, 4), dtype=np.uint8)
    for i, pr in enumerate(proofs):
        b = np.frombuffer(pr, dtype=np.uint8)[:stride]
        buf[i * stride:i * stride + len(b)] = b
    lens = p3.dev_u32(np.array([len(pr) for pr in proofs], dtype=np.uint32)) if with_lens else None
    d_pis = p3.dev_u32(np.ascontiguousarray(pis, dtype=np.uint32).reshape(-1)) if v.n_public else None
    status, rejected = DB.guarded(n, offset_words=1), DB.guarded(1, offset_words=3)
    v.verify_many_dev(torch.from_numpy(buf).cuda(), d_pis, lens=lens, n=n, stride=stride, status=status.view, rejected=rejected.view if count else False)
    torch.cuda.synchronize()
    status.assert_guards_intact("d_status")
    rejected.assert_guards_intact("d_rejected")
    status.assert_fully_written("d_status")
    if not count:
        assert rejected.host()[0] == DB.SENTINEL
    return status.host(), (int(rejected.host()[0]) if count else None)


# ---- 1. accept --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,kind", AM.HASHES)
@pytest.mark.parametrize("name", AM.NAMES)
def test_accepts_reference_and_device_proofs_in_one_batch(p3, airs, name, hash, kind):
    """A verifier serves one log_n: at log_n 3 and at log_n 5 one batch holds proofs of the CPU reference prover (even members) and of
    prove_air (odd members), every member another instance with its own public values."""
    air, gen = airs[name]
    t = FRI[name]
    fp = p3.FriParameters(*t)
    for log_n in (3, 5):
        proofs, pis = [], []
        for j, args in enumerate(INSTANCES[name]):
            if j % 2 == 0:
                pr, pi = AM.ref_proof(airs, name, kind, log_n, t, **args)
            else:
                trace, pi = gen(log_n, **args)
                pr = gpu_proof(p3, air, trace, pi, hash, t)
            assert air.verify(pr, pi, log_n, fp, hash) == 0
            proofs.append(pr)
            pis.append(pi)
        v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=len(proofs))
        assert all(len(pr) == v.proof_len for pr in proofs)
        st, rej = dev_entry(p3, v, proofs, np.stack(pis))
        assert not st.any() and rej == 0, (name, hash, log_n, st, rej)
        assert not v.verify_many(proofs, np.stack(pis)).any()
        v.close()


# ---- 2. out-of-domain evaluation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash,kind", AM.HASHES)
@pytest.mark.parametrize("name", AM.NAMES)
def test_broken_traces_and_foreign_public_values_are_ood_mismatches(p3, airs, name, hash, kind):
    air, gen = airs[name]
    t, log_n = FRI[name], 4
    fp = p3.FriParameters(*t)
    made = []
    for args in INSTANCES[name][:3]:
        trace, pi = gen(log_n, **args)
        made.append((trace, pi, gpu_proof(p3, air, trace, pi, hash, t)))
    broken = made[0][0].copy()
    broken[5, 0] = (int(broken[5, 0]) + 1) % P  # one transition no longer holds; the prover does not judge
    bad = gpu_proof(p3, air, broken, made[0][1], hash, t)
    proofs = [made[0][2], bad, made[1][2], made[2][2], made[1][2], made[0][2]]
    pis = [made[0][1], made[0][1], made[1][1], made[1][1], made[2][1], made[0][1]]  # members 3 and 4: another member's public values
    want = [AM.host_code(air, pr, pi, log_n, fp, hash) for pr, pi in zip(proofs, pis)]
    assert want == [0, 10, 0, 10, 10, 0]
    v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=8)
    st, rej = dev_entry(p3, v, proofs, np.stack(pis))
    assert list(st) == want and rej == 3, (st, rej)
    assert list(v.verify_many(proofs, np.stack(pis))) == want
    v.close()


# ---- 3. tamper sweep ----------------------------------------------------------------------------------------------------------------
SWEEP_FRI = {"fib": (1, 0, 2, 2), "D": (3, 0, 2, 1)}  # two queries of 3 / 5 index bits: a search finds a final polynomial the indices survive


def _search(air, good, pis, log_n, fp, hash, off, code):
    """the first change of word `off` for which the host verifier answers `code`"""
    orig = int(np.frombuffer(good, dtype=np.uint32)[off])
    for k in range(1, 60000):
        bad = AM.with_word(good, off, (orig + k) % P)
        if air.verify(bad, pis, log_n, fp, hash) == code:
            return bad
    raise AssertionError("no change of word %d gives code %d" % (off, code))


@pytest.mark.parametrize("hash,kind", AM.HASHES)
@pytest.mark.parametrize("name", ["fib", "D"])
def test_tamper_sweep_against_the_host_verifier(p3, airs, name, hash, kind):
    air = airs[name][0]
    t, log_n = SWEEP_FRI[name], 2
    fp = p3.FriParameters(*t)
    w, C = air.width, air.n_chunks
    base = [AM.ref_proof(airs, name, kind, log_n, t, **args) for args in INSTANCES[name]]
    good, gpis = base[0]
    classes = AM.word_classes(kind, t, log_n, w, C)
    nw, head = len(classes), A.header_words(w, air.log_quotient_degree)
    assert 4 * nw == len(good)
    hk = AM.header_kinds(w, C)
    rng = np.random.default_rng(900 + 2 * len(name) + kind)
    pick = lambda offs: int(offs[int(rng.integers(len(offs)))])
    fri = lambda cls: head + np.nonzero(classes[head:] == cls)[0]
    bad = [(k, AM.with_word(good, hk[k][0])) for k in ("magic", "version", "log_n")]
    bad += [("count %d" % o, AM.with_word(good, o)) for o in hk["count"]]
    bad += [(k, AM.with_word(good, pick(hk[k]))) for k in ("root", "local", "next", "chunk")]
    bad += [("FRI class %d" % cls, AM.with_word(good, pick(fri(cls)))) for cls in (M.SHAPE, M.FELT, M.DIGEST) if len(fri(cls))]
    bad += [("FRI word %d" % o, AM.with_word(good, o)) for o in sorted(set(int(o) for o in rng.integers(head, nw, 40)))]
    bad += [("FRI shape word %d" % o, AM.with_word(good, int(o))) for o in fri(M.SHAPE)[:12]]
    bad += [(k + " = P", AM.with_word(good, pick(hk[k]), P)) for k in ("root", "local", "next", "chunk")]
    bad += [("FRI field word %d = P" % o, AM.with_word(good, o, P)) for o in (int(fri(M.FELT)[0]), pick(fri(M.FELT)), nw - 1)]
    bad += [("four bytes short", good[:-4]), ("four bytes long", good + b"\0\0\0\0")]
    both = AM.with_word(AM.with_word(good, hk["local"][0]), head)  # a header value AND the FRI section's first count word
    bad += [("header value and FRI count", both)]
    bad += [("witness", _search(air, good, gpis, log_n, fp, hash, nw - 1, 11)), ("final polynomial", _search(air, good, gpis, log_n, fp, hash, nw - 5, 15))]
    proofs, pis, want, whats = [], [], [], []
    for j, (what, pr) in enumerate(bad):  # untouched members interleaved
        u, upi = base[j % len(base)]
        proofs += [u, pr]
        pis += [upi, gpis]
        want += [0, AM.expected_status(AM.host_code(air, pr, gpis, log_n, fp, hash), pr, gpis, classes, good)]
        whats += ["untouched", what]
    proofs.append(good), pis.append(gpis), want.append(0), whats.append("untouched")
    assert all(AM.host_code(air, pr, pi, log_n, fp, hash) == 0 for pr, pi, wh in zip(proofs, pis, whats) if wh == "untouched")
    assert want[whats.index("header value and FRI count")] == AM.MALFORMED
    assert {0, 10, 11, 13, 14, 15, 16} <= set(want), sorted(set(want))  # the sweep is not vacuous
    v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=len(proofs))
    st, rej = dev_entry(p3, v, proofs, np.stack(pis))
    wrong = [(wh, int(s), e) for wh, s, e in zip(whats, st, want) if s != e]
    assert not wrong, "(what, status, the contract's): %s" % wrong
    assert rej == sum(1 for e in want if e)
    v.close()
    v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=16)  # the host entry, in rounds
    assert list(v.verify_many(proofs, np.stack(pis))) == want
    v.close()


# ---- 4. geometry and contract -------------------------------------------------------------------------------------------------------
def _no_publics(p3):
    """width 2, no public value, degree 3: next.x = x y; next.y = y + 1; first row y = 2"""
    b = p3.AirBuilder(2, 0)
    x, y = b.local(0), b.local(1)
    tr = b.when_transition()
    tr.assert_eq(b.next(0), x * y)
    tr.assert_eq(b.next(1), y + b.const(1))
    b.when_first_row().assert_eq(y, b.const(2))
    return b.build()


def _trace_no_publics(log_n, x0=3):
    rows, (x, y) = [], (x0 % P, 2)
    for _ in range(1 << log_n):
        rows.append((x, y))
        x, y = x * y % P, (y + 1) % P
    return M.R.O.to_monty(np.array(rows, dtype=np.uint64))


@pytest.mark.parametrize("hash,kind", AM.HASHES)
def test_batch_geometry_and_refusals(p3, airs, hash, kind):
    import torch
    air = airs["fib"][0]
    t, log_n = FRI["fib"], 3
    fp = p3.FriParameters(*t)
    base = [AM.ref_proof(airs, "fib", kind, log_n, t, **args) for args in INSTANCES["fib"]]
    classes = AM.word_classes(kind, t, log_n, air.width, air.n_chunks)
    proofs, pis, want = [], [], []
    for j in range(7):  # accepted and rejected members interleaved
        pr, pi = base[j % 4]
        if j % 3 == 1:
            pr = AM.with_word(pr, int(np.nonzero(classes != M.SHAPE)[0][(53 * j) % int((classes != M.SHAPE).sum())]))
        proofs.append(pr), pis.append(pi)
        want.append(AM.expected_status(AM.host_code(air, pr, pi, log_n, fp, hash), pr, pi, classes, base[0][0]))
    pis = np.stack(pis)
    assert want.count(0) == 5
    v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=7)
    for with_lens, pad in ((True, 0), (False, 0), (True, 20), (False, 20)):  # n = max_proofs; the stride above the length; d_lens given or not
        st, rej = dev_entry(p3, v, proofs, pis, with_lens, pad)
        assert list(st) == want and rej == 2, (with_lens, pad, st)
    st, rej = dev_entry(p3, v, proofs[1:2], pis[1:2])  # n = 1, a rejected member, back to back on one verifier
    assert list(st) == want[1:2] and rej == 1
    st, rej = dev_entry(p3, v, proofs[:1], pis[:1])
    assert list(st) == [0] and rej == 0
    st, rej = dev_entry(p3, v, proofs, pis, count=False)  # d_rejected NULL
    assert list(st) == want and rej is None
    v.close()
    v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=3)
    assert list(v.verify_many(proofs, pis)) == want  # 7 members in rounds of 3
    # batch-level faults are refused before any launch: nothing is written
    n = 2
    buf = torch.zeros(4 * v.proof_len + 8, dtype=torch.uint8, device="cuda")
    d_pis = p3.dev_u32(pis[:4].reshape(-1))
    status, rejected = DB.guarded(4), DB.guarded(1)
    call = lambda b, n, stride: v.verify_many_dev(b, d_pis, n=n, stride=stride, status=status.view, rejected=rejected.view)
    for b, m, stride, msg in ((buf, n, v.proof_len - 4, "stride"), (buf, n, v.proof_len + 2, "stride"), (buf[1:], n, v.proof_len, "aligned"),
                              (buf, 4, v.proof_len, "more proofs than the verifier was created for")):
        with pytest.raises(p3.P3HipError, match=msg) as e:
            call(b, m, stride)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert (status.host() == DB.SENTINEL).all() and (rejected.host() == DB.SENTINEL).all()
    v.close()


@pytest.mark.parametrize("hash,kind", AM.HASHES)
def test_an_air_without_public_values_takes_no_d_pis(p3, oracle, hash, kind):
    air = _no_publics(p3)
    assert air.n_public == 0 and air.log_quotient_degree == 1
    t, log_n = (1, 0, 3, 1), 3
    fp = p3.FriParameters(*t)
    proofs = [gpu_proof(p3, air, _trace_no_publics(log_n, x0), None, hash, t) for x0 in (3, 5, P - 1)]
    broken = _trace_no_publics(log_n)
    broken[2, 1] = (int(broken[2, 1]) + 1) % P
    proofs.insert(1, gpu_proof(p3, air, broken, None, hash, t))
    want = [AM.host_code(air, pr, None, log_n, fp, hash) for pr in proofs]
    assert want == [0, 10, 0, 0]
    v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=4)
    air.free()  # the verifier holds its own copy of the program
    st, rej = dev_entry(p3, v, proofs, None)
    assert list(st) == want and rej == 1
    assert list(v.verify_many(proofs, None)) == want
    v.close()


# ---- 5. lifetime --------------------------------------------------------------------------------------------------------------------
def test_fifty_create_verify_destroy_cycles_with_the_air_destroyed_at_once(p3, airs):
    import psutil
    import torch
    t, log_n = FRI["B"], 3
    fp = p3.FriParameters(*t)
    src = airs["B"][0]
    members = [AM.ref_proof(airs, "B", kind, log_n, t, **args) for kind in (0, 1) for args in INSTANCES["B"][:2]]
    tampered = AM.with_word(members[0][0], 25)  # a local value: OodEvaluationMismatch

    def cycle():
        for kind, hash in ((0, "poseidon2"), (1, "keccak")):
            air = p3.Air(src.width, src.n_public, src.code, src.consts)
            v = p3.AirVerifier(air, log_n, fp, hash, max_proofs=4)
            air.free()  # right after create
            mine = members[2 * kind:2 * kind + 2]
            proofs, pis = [m[0] for m in mine] + ([tampered] if kind == 0 else []), np.stack([m[1] for m in mine] + ([members[0][1]] if kind == 0 else []))
            want = [0, 0] + ([10] if kind == 0 else [])
            assert list(v.verify_many(proofs, pis)) == want
            assert list(dev_entry(p3, v, proofs, pis)[0]) == want
            v.close()
        gc.collect()
        torch.cuda.empty_cache()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    for _ in range(3):
        cycle()
    me = psutil.Process()
    base, rss0 = free_bytes(), me.memory_info().rss
    for _ in range(50):
        cycle()
    lost, grown = base - free_bytes(), me.memory_info().rss - rss0
    MIB = 1 << 20
    # 100 verifiers with some thirty device buffers and a stream each (the owned PCS verifier's included): the smallest leaked buffer
    # costs a 2 MiB granule per cycle, 100 MiB over the 50
    assert lost < 8 * MIB, "free device memory fell by %.1f MiB over 50 create / verify / destroy cycles" % (lost / MIB)
    assert grown < 64 * MIB, "resident host memory grew by %.1f MiB over 50 create / verify / destroy cycles" % (grown / MIB)
