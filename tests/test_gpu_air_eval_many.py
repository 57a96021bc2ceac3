"""GPU tests of p3hip_air_eval_ext_dev (include/p3hip.h; csrc/air_verifier_dev.hip air_eval_core, the interpreter of the batch
verifier's av_eval_kernel): the program over extension operands at n points, one lane per point, word for word against
air_ref.eval_ext.  The reference for many points is air_ref.run — the walker eval_ext itself runs — over a numpy ring that holds
every point at once; it is pinned to air_ref.eval_ext at the first and the last point of every case."""
import numpy as np
import pytest

import air_fuzz as F
import air_ref as A
import dev_buffers as DB
import pcs_ref as R

pytestmark = pytest.mark.gpu
P = R.P
NS = (1, 63, 64, 65, 130)  # a partial wave, the workgroup edge, a second workgroup with a partial tail
FUZZ = (3, 13, 26, 39, 47, 48)  # every degree, slot spans 64 / 2 / 8 / 64 / 64, and a program that asserts leaves only (no slot)


# ---- the extension ring over (n, 4) arrays of canonical uint64 ----
def _mul(a, b):
    a, b = np.broadcast_arrays(a, b)
    out = np.zeros(a.shape, dtype=np.uint64)
    for i in range(4):
        for j in range(4):
            t = a[..., i] * b[..., j] % P
            out[..., (i + j) & 3] = (out[..., (i + j) & 3] + (t * 11 if i + j >= 4 else t)) % P
    return out


_RING = (lambda a, b: (a + b) % P, lambda a, b: (a + P - b) % P, _mul)


def eval_ext_many(code, consts, local, nxt, pis, sels, alpha):
    """Montgomery words in and out: local, nxt (n, width, 4); pis (n, n_public); sels (n, 3, 4); alpha (n, 4) -> (n, 4)"""
    c = lambda v: R.O.from_monty(np.asarray(v, dtype=np.uint32)).astype(np.uint64)
    local, nxt, pis, sels, alpha, consts = c(local), c(nxt), c(pis), c(sels), c(alpha), c(consts)
    n = len(alpha)
    base = lambda col: np.concatenate([col.reshape(-1, 1), np.zeros((len(col), 3), dtype=np.uint64)], axis=1)
    tables = {A.LOCAL: lambda i: local[:, i], A.NEXT: lambda i: nxt[:, i], A.PUBLIC: lambda i: base(pis[:, i]),
              A.CONST: lambda i: base(np.full(n, consts[i], dtype=np.uint64)), A.SELECTOR: lambda i: sels[:, i]}
    acc = np.zeros((n, 4), dtype=np.uint64)
    for v in A.run(code, lambda kind, idx: tables[kind](idx), _RING):
        acc = (_mul(acc, alpha) + v) % P
    return R.O.to_monty(acc)


def _operands(rng, n, width, n_public):
    """canonical values with 0 and P - 1 among them: point 0 all zero, point 1 all P - 1, a tenth of the rest one of the two"""
    def draw(*shape):
        v = rng.integers(0, P, shape, dtype=np.uint64)
        special = rng.random(shape) < 0.1
        v[special] = np.where(rng.random(shape) < 0.5, 0, P - 1)[special]
        v[0] = 0
        if n > 1:
            v[1] = P - 1
        return R.O.to_monty(v)
    return draw(n, width, 4), draw(n, width, 4), draw(n, max(n_public, 1))[:, :n_public], draw(n, 3, 4), draw(n, 4)


def _check(p3, air, code, consts, what, ns=NS, seed=0):
    import torch
    rng = np.random.default_rng([0xE7A1, seed])
    for n in ns:
        local, nxt, pis, sels, alpha = _operands(rng, n, air.width, air.n_public)
        want = eval_ext_many(code, consts, local, nxt, pis, sels, alpha)
        for k in {0, n - 1}:
            assert np.array_equal(want[k], A.eval_ext(code, consts, local[k], nxt[k], pis[k], sels[k], alpha[k])), (what, n, k)
        # every buffer 4-byte aligned and no more: an odd number of words past a 512-byte boundary
        ins = [DB.place(v, offset_words=o) for v, o in ((local, 1), (nxt, 3), (pis if air.n_public else np.zeros(1, np.uint32), 5), (sels, 7), (alpha, 9))]
        out = DB.guarded(4 * n, offset_words=11)
        got = air.eval_ext_many(ins[0].view, ins[1].view, ins[2].view if air.n_public else None, ins[3].view, ins[4].view, out=out.view)
        torch.cuda.synchronize()
        out.assert_guards_intact("d_out of %s at n = %d" % (what, n))
        out.assert_fully_written("d_out")
        for b in ins:
            b.assert_unchanged("an input of %s" % what)
        assert np.array_equal(p3.host_u32(got).reshape(n, 4), want), (what, n)
        assert np.array_equal(out.host().reshape(n, 4), want)


@pytest.fixture(scope="module")
def airs(p3, oracle):
    return A.all_airs(p3)


@pytest.mark.parametrize("name", ["fib", "B", "C", "D"])
def test_the_four_airs_at_every_batch_geometry(p3, airs, name):
    air = airs[name][0]
    _check(p3, air, air.code, air.consts, name, seed=len(name))


@pytest.mark.parametrize("index", FUZZ)
def test_raw_programs_at_every_batch_geometry(p3, oracle, index):
    case = F.FUZZ_CASES[index]
    air = case.air(p3)
    assert air.n_slots == case.n_slots
    _check(p3, air, case.code, case.consts, repr(case), seed=index)
    air.free()


def test_the_capacity_program_fills_64_slots_of_lds(p3, oracle):
    """width 8192, 4096 public values, 65536 constants, 65536 instructions, 4096 constraints, 64 slots: 64 KiB of LDS per workgroup.
    n = 65: two workgroups, the second with one lane."""
    code, consts = F.capacity_program()
    air = p3.Air(F.CAP_WIDTH, F.CAP_PUBLIC, code, consts)
    assert air.n_slots == A.MAX_SLOTS
    _check(p3, air, code, consts, "the capacity program", ns=(65,), seed=64)
    air.free()


def test_no_points_is_no_operation_and_too_many_are_refused(p3, airs):
    import ctypes as C
    import torch
    air = airs["B"][0]
    out = DB.guarded(4)
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    air.eval_ext_many(empty, empty, empty, empty, empty, out=out.view)
    torch.cuda.synchronize()
    assert (out.host() == DB.SENTINEL).all()
    out.assert_guards_intact("d_out")
    p = C.c_void_p(out.data_ptr())
    rc = p3._lib.lib().p3hip_air_eval_ext_dev(air._h, None, p, p, p, p, p, (1 << 20) + 1, p)  # refused before anything is read or launched
    assert rc == -1 and "at most 2^20" in p3.take_last_error()
    torch.cuda.synchronize()
    assert (out.host() == DB.SENTINEL).all()
