"""Caller-defined AIRs (include/p3hip.h "caller-defined AIRs"): AirBuilder, shaped after p3_air::AirBuilder, records an AIR's
constraints as an expression DAG and compiles it to the library's instruction list; Air owns the validated program and runs it —
quotient_values and check_constraints on the device, the verifier's evaluation on the host; prove_air / verify_air are
p3_uni_stark::prove / verify over a non-hiding TwoAdicFriPcs and a Challenger; AirProver is the same prover as one device-resident
launch chain of the library's.  Field elements are Montgomery words unless said
otherwise.  There is no CPU path for the device steps."""
import ctypes as C

import numpy as np

from . import _lib
from .fib_air import VERIFY_MALFORMED, FriParameters, _hash_kind, profile_kind
from .gpu_dft import P, _is_torch, _stream_ptr, dev_u32
from .pcs import Challenger, PcsRejected, _words

# include/p3hip.h P3HIP_AIR_*
OP_ADD, OP_SUB, OP_MUL, OP_ASSERT_ZERO = 0, 1, 2, 3
KIND_SHIFT = 24
KIND_SLOT, KIND_LOCAL, KIND_NEXT, KIND_PUBLIC, KIND_CONST, KIND_SELECTOR = range(6)
SEL_FIRST_ROW, SEL_LAST_ROW, SEL_TRANSITION = 0, 1, 2
MAX_INSTRUCTIONS, MAX_CONSTRAINTS, MAX_SLOTS, MAX_WIDTH, MAX_PUBLIC, MAX_CONSTS, MAX_DEGREE = 65536, 4096, 64, 8192, 4096, 65536, 9
PROOF_MAGIC = 0x42463350
OOD_EVALUATION_MISMATCH = 10

_R = (1 << 32) % P
_RINV = pow(_R, P - 2, P)


def to_monty(v):
    return (int(v) % P) * _R % P


def from_monty(w):
    return int(w) * _RINV % P


def two_adic_generator(bits):
    """(31^15)^(2^(27 - bits)), a Montgomery word"""
    return to_monty(pow(pow(31, 15, P), 1 << (27 - bits), P))


def operand(kind, index):
    return (kind << KIND_SHIFT) | index


# ---- expressions ----
class Expr:
    """A node of an AirBuilder's DAG.  + - * take expressions or canonical integers."""
    __slots__ = ("b", "id")

    def __init__(self, builder, node_id):
        self.b, self.id = builder, node_id

    def _lift(self, other):
        if isinstance(other, Expr):
            if other.b is not self.b:
                raise ValueError("expressions of two builders")
            return other
        return self.b.const(other)

    def __add__(self, o):
        return self.b._binary(OP_ADD, self, self._lift(o))

    def __radd__(self, o):
        return self.b._binary(OP_ADD, self._lift(o), self)

    def __sub__(self, o):
        return self.b._binary(OP_SUB, self, self._lift(o))

    def __rsub__(self, o):
        return self.b._binary(OP_SUB, self._lift(o), self)

    def __mul__(self, o):
        return self.b._binary(OP_MUL, self, self._lift(o))

    def __rmul__(self, o):
        return self.b._binary(OP_MUL, self._lift(o), self)

    def __neg__(self):
        return self.b._binary(OP_SUB, self.b.const(0), self)


class _Filtered:
    """p3_air::FilteredAirBuilder: every assertion is multiplied by the condition."""

    def __init__(self, builder, condition):
        self._b, self._c = builder, condition

    def assert_zero(self, e):
        self._b.assert_zero(self._c * e)

    def assert_eq(self, a, b):
        self.assert_zero(self._b._expr(a) - b)


class AirBuilder:
    """Records constraints over a base-field trace of `width` columns with `n_public` public values; build() gives the Air."""

    def __init__(self, width, n_public=0):
        self.width, self.n_public = int(width), int(n_public)
        self._nodes, self._ids, self._asserts = [], {}, []  # node: (kind, index) for a leaf, (op, a id, b id) otherwise
        self._consts, self._const_ids = [], {}

    def _leaf(self, kind, index):
        return self._node(("leaf", kind, index))

    def _node(self, key):
        i = self._ids.get(key)
        if i is None:
            i = self._ids[key] = len(self._nodes)
            self._nodes.append(key)
        return Expr(self, i)

    def _binary(self, op, a, b):
        ia, ib = a.id, b.id
        if op != OP_SUB and ia > ib:  # a + b and b + a are one node
            ia, ib = ib, ia
        return self._node(("op", op, ia, ib))

    def _expr(self, e):
        return e if isinstance(e, Expr) else self.const(e)

    def local(self, c):
        if not 0 <= c < self.width:
            raise IndexError("column %d of a trace of width %d" % (c, self.width))
        return self._leaf(KIND_LOCAL, int(c))

    def next(self, c):
        if not 0 <= c < self.width:
            raise IndexError("column %d of a trace of width %d" % (c, self.width))
        return self._leaf(KIND_NEXT, int(c))

    def public(self, i):
        if not 0 <= i < self.n_public:
            raise IndexError("public value %d of %d" % (i, self.n_public))
        return self._leaf(KIND_PUBLIC, int(i))

    def const(self, v):
        """a constant from a canonical integer (taken mod P)"""
        w = to_monty(v)
        i = self._const_ids.get(w)
        if i is None:
            i = self._const_ids[w] = len(self._consts)
            self._consts.append(w)
        return self._leaf(KIND_CONST, i)

    @property
    def is_first_row(self):
        return self._leaf(KIND_SELECTOR, SEL_FIRST_ROW)

    @property
    def is_last_row(self):
        return self._leaf(KIND_SELECTOR, SEL_LAST_ROW)

    @property
    def is_transition(self):
        return self._leaf(KIND_SELECTOR, SEL_TRANSITION)

    def assert_zero(self, e):
        self._asserts.append(self._expr(e).id)

    def assert_eq(self, a, b):
        self.assert_zero(self._expr(a) - b)

    def when_first_row(self):
        return _Filtered(self, self.is_first_row)

    def when_last_row(self):
        return _Filtered(self, self.is_last_row)

    def when_transition(self):
        return _Filtered(self, self.is_transition)

    def compile(self):
        """-> (code as numpy uint32 (n, 4), consts as numpy uint32).  Every DAG node is emitted once, in the order the constraints
        first need it; a slot is handed back after its value's last use and taken again by a later instruction."""
        nodes = self._nodes
        order, seen = [], set()  # ("op", node) | ("assert", node)
        for root in self._asserts:
            stack = [(root, False)]
            while stack:  # post-order without recursion: a chain may be thousands of nodes deep
                v, done = stack.pop()
                if nodes[v][0] == "leaf" or (v in seen and not done):
                    continue
                if done:
                    order.append(("op", v))
                    continue
                seen.add(v)
                stack.append((v, True))
                stack.append((nodes[v][3], False))
                stack.append((nodes[v][2], False))
            order.append(("assert", root))
        last_use = {}
        for pos, (what, v) in enumerate(order):
            for u in ([v] if what == "assert" else nodes[v][2:4]):
                last_use[u] = pos
        slot_of, free, n_slots, code = {}, [], 0, []

        def opnd(u):
            if nodes[u][0] == "leaf":
                return operand(nodes[u][1], nodes[u][2])
            return operand(KIND_SLOT, slot_of[u])

        def release(u, pos):
            if nodes[u][0] == "op" and last_use[u] == pos and u in slot_of:
                free.append(slot_of.pop(u))

        for pos, (what, v) in enumerate(order):
            if what == "assert":
                code.append((OP_ASSERT_ZERO, 0, opnd(v), 0))
                release(v, pos)
                continue
            _, op, a, b = nodes[v]
            oa, ob = opnd(a), opnd(b)
            release(a, pos)
            release(b, pos)  # dst may be an operand's slot: a lane reads both operands before it writes
            if v in last_use:
                if free:
                    s = min(free)
                    free.remove(s)
                else:
                    s, n_slots = n_slots, n_slots + 1
                slot_of[v] = s
                code.append((op, s, oa, ob))
        return np.array(code, dtype=np.uint32).reshape(-1, 4), np.array(self._consts, dtype=np.uint32)

    def build(self):
        code, consts = self.compile()
        return Air(self.width, self.n_public, code, consts)


class _Info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "n_public", "n_instructions", "n_constraints", "n_slots", "max_degree", "log_quotient_degree")]


class Air:
    """A validated AIR program (p3hip_air_create; refusals raise P3HipError(-1) naming the instruction).  Owns the handle."""

    def __init__(self, width, n_public, code, consts):
        self.code = np.ascontiguousarray(code, dtype=np.uint32).reshape(-1, 4)
        self.consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().p3hip_air_create(int(width), int(n_public), self.code.ctypes.data_as(C.c_void_p), len(self.code),
                                               self.consts.ctypes.data_as(C.c_void_p), self.consts.size, C.byref(self._h)))
        info = _Info()
        _lib.check(_lib.lib().p3hip_air_info(self._h, C.byref(info)))
        self.width, self.n_public, self.n_instructions = info.width, info.n_public, info.n_instructions
        self.n_constraints, self.n_slots, self.max_degree = info.n_constraints, info.n_slots, info.max_degree
        self.log_quotient_degree = info.log_quotient_degree

    @property
    def n_chunks(self):
        return 1 << self.log_quotient_degree

    def _pis(self, pis):
        p = _words(pis if pis is not None else [], self.n_public)
        return p, (p.ctypes.data_as(C.c_void_p) if p.size else None)

    def quotient(self, lde, log_n, log_blowup, pis, alpha):
        """quotient_values: lde the committed trace LDE (TwoAdicFriPcs.get_evaluations_on_domain, any number of its rows from
        2^(log_n + log_quotient_degree) on; read in place) -> the n_chunks chunk matrices, (2^log_n, 4) int32 device tensors; chunk
        c is committed with domain shift GENERATOR g_qn^c.  Enqueued on torch's current stream, not synchronised."""
        import torch
        if not (lde.is_cuda and lde.is_contiguous() and lde.element_size() == 4 and lde.dim() == 2 and lde.shape[1] == self.width):
            raise ValueError("quotient: a contiguous (rows, width) device matrix of 32-bit words")
        if lde.shape[0] < (1 << (log_n + self.log_quotient_degree)):
            raise ValueError("quotient: the LDE holds fewer rows than the quotient domain")
        p, pp = self._pis(pis)
        al = _words(alpha, 4)
        chunks = [torch.empty((1 << log_n, 4), dtype=torch.int32, device=lde.device) for _ in range(self.n_chunks)]
        ptrs = (C.c_void_p * self.n_chunks)(*[c.data_ptr() for c in chunks])
        _lib.check(_lib.lib().p3hip_air_quotient_dev(self._h, _stream_ptr(), C.c_void_p(lde.data_ptr()), log_n, log_blowup, pp,
                                                     al.ctypes.data_as(C.c_void_p), ptrs))
        return chunks

    def check_trace(self, trace, pis=None):
        """check_constraints: trace a (2^log_n, width) device tensor (read in place) or numpy array (uploaded) -> None when every
        constraint holds on every row, else the smallest failing (row, constraint)."""
        t = trace.contiguous() if _is_torch(trace) else dev_u32(trace)
        h = int(t.shape[0]) if t.dim() == 2 else 0
        if t.dim() != 2 or t.element_size() != 4 or not t.is_cuda or t.shape[1] != self.width or h < 2 or h & (h - 1):
            raise ValueError("check_trace: a (2^log_n, width) matrix of 32-bit words, log_n >= 1")
        p, pp = self._pis(pis)
        row, k = C.c_longlong(), C.c_int()
        _lib.check(_lib.lib().p3hip_air_check_trace_dev(self._h, _stream_ptr(), C.c_void_p(t.data_ptr()), h.bit_length() - 1, pp,
                                                        C.byref(row), C.byref(k)))
        return None if row.value < 0 else (row.value, k.value)

    def eval_ext(self, local, next, pis, sels, alpha):
        """The constraints at a point, folded by Horner's rule (host): local, next (width, 4); sels (3, 4): is_first_row,
        is_last_row, is_transition -> 4 words."""
        lo, nx = _words(local, 4 * self.width), _words(next, 4 * self.width)
        p, pp = self._pis(pis)
        s, al, out = _words(sels, 12), _words(alpha, 4), np.zeros(4, dtype=np.uint32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.lib().p3hip_air_eval_ext(self._h, vp(lo), vp(nx), pp, vp(s), vp(al), vp(out)))
        return out

    def eval_ext_many(self, local, next, pis, sels, alpha, out=None):
        """eval_ext at n points in one launch, one lane per point (p3hip_air_eval_ext_dev): contiguous 32-bit device tensors of n x
        width x 4, n x width x 4, n x n_public (None when the AIR has no public values), n x 12 and n x 4 canonical Montgomery words ->
        an (n, 4) int32 device tensor (or `out`, of which 4 n words are written).  Enqueued on torch's current stream, not
        synchronised; at most 2^20 points a call."""
        import torch
        n = int(alpha.numel()) // 4
        need = [(local, 4 * self.width * n), (next, 4 * self.width * n), (sels, 12 * n), (alpha, 4 * n)] + ([(pis, self.n_public * n)] if self.n_public else [])
        for t, words in need:
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != 4 or t.numel() != words:
                raise ValueError("eval_ext_many: contiguous device tensors of 32-bit words, one row per point")
        if out is None:
            out = torch.empty((max(n, 1), 4), dtype=torch.int32, device=alpha.device)
        elif not out.is_cuda or not out.is_contiguous() or out.element_size() != 4 or out.numel() < 4 * n:
            raise ValueError("eval_ext_many: out must hold 4 words per point")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().p3hip_air_eval_ext_dev(self._h, _stream_ptr(), ptr(local), ptr(next), ptr(pis) if self.n_public else None, ptr(sels),
                                                     ptr(alpha), n, ptr(out)))
        return out.reshape(-1, 4)[:n]

    def verify(self, proof, pis, log_n, params, hash="poseidon2"):
        """p3_uni_stark::verify for one proof, the library's host verifier (p3hip_air_verify): 0 = accept, else the code AirRejected
        carries (1-4 header, 10 OodEvaluationMismatch, the PCS verifier's otherwise).  A refused argument raises P3HipError(-1)."""
        p, pp = self._pis(pis)
        buf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(bytes(proof) or b"\0")
        code = C.c_int()
        _lib.check(_lib.lib().p3hip_air_verify(self._h, _hash_kind(hash), int(log_n), C.cast(params._c(), C.c_void_p), buf, len(proof), pp, C.byref(code)))
        if code.value:
            _lib.take_last_error()
        return code.value

    def free(self):
        if self._h:
            _lib.lib().p3hip_air_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def fibonacci_air():
    """FibonacciAir (native/src/fib_air.rs:224-264): columns (left, right), publics (a, b, x); five constraints."""
    b = AirBuilder(2, 3)
    left, right, nleft, nright = b.local(0), b.local(1), b.next(0), b.next(1)
    first = b.when_first_row()
    first.assert_eq(left, b.public(0))
    first.assert_eq(right, b.public(1))
    trans = b.when_transition()
    trans.assert_eq(right, nleft)
    trans.assert_eq(left + right, nright)
    b.when_last_row().assert_eq(right, b.public(2))
    return b.build()


# ---- extension field on the host (canonical integers; x^4 = 11): the few operations verify_air needs ----
def _emul(a, b):
    out = [0, 0, 0, 0]
    for i in range(4):
        for j in range(4):
            t = a[i] * b[j]
            out[(i + j) & 3] += t * 11 if i + j >= 4 else t
    return [v % P for v in out]


def _eadd(a, b):
    return [(x + y) % P for x, y in zip(a, b)]


def _esub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def _base(v):
    return [v % P, 0, 0, 0]


def _epow(a, e):
    r = _base(1)
    while e:
        if e & 1:
            r = _emul(r, a)
        a = _emul(a, a)
        e >>= 1
    return r


def _einv(a):
    conj = [a[0], -a[1] % P, a[2], -a[3] % P]
    n = _emul(a, conj)  # c + d x^2
    c, d = n[0], n[2]
    di = pow((c * c - 11 * d * d) % P, P - 2, P)
    return _emul(conj, [c * di % P, 0, -d * di % P, 0])


def _canon(words):
    return [from_monty(w) for w in words]


def _monty(vals):
    return np.array([to_monty(v) for v in vals], dtype=np.uint32)


# ---- p3_uni_stark::prove / verify ----
def _prefix(ch, log_n, root_t, pis):
    m = to_monty(log_n)
    ch.observe([m, m])  # log_ext_degree, log_degree
    ch.observe_digest(root_t)
    if len(pis):
        ch.observe(pis)
    return ch.sample_ext()


def chunk_shifts(log_n, log_quotient_degree):
    """the domain shift of every quotient chunk: GENERATOR g_qn^c"""
    g, s, out = from_monty(two_adic_generator(log_n + log_quotient_degree)), 31, []
    for _ in range(1 << log_quotient_degree):
        out.append(to_monty(s))
        s = s * g % P
    return out


def prove_air(air, pcs, trace, pis=None):
    """p3_uni_stark::prove(&config, &air, trace, &pis) over a non-hiding TwoAdicFriPcs: trace a (2^log_n, width) device tensor
    (committed where it lies) or numpy array.  Returns the proof bytes: the header (magic, 1, log_n, the two roots, width and the
    local values, width and the next values, the chunk count and per chunk 4 and its values), then the PCS's FriProof bytes.  The
    host drives the challenger, so the call synchronises a few times (two commits, the open)."""
    if getattr(pcs, "_hiding", False):
        raise ValueError("prove_air: a non-hiding TwoAdicFriPcs")
    pis = _words(pis if pis is not None else [], air.n_public)
    h, w = (int(v) for v in trace.shape)
    log_n = h.bit_length() - 1
    if w != air.width or h < 2 or h & (h - 1):
        raise ValueError("prove_air: a (2^log_n, %d) trace, log_n >= 1" % air.width)
    lqd = air.log_quotient_degree
    if pcs.params.log_blowup < lqd:
        raise ValueError("prove_air: log_blowup %d is below the AIR's log_quotient_degree %d" % (pcs.params.log_blowup, lqd))
    root_t, data_t = pcs.commit([(trace, None)])
    ch, data_q = Challenger(pcs.hash), None
    try:  # the trees and LDEs go back to the device whatever happens below
        alpha = _prefix(ch, log_n, root_t, pis)
        lde = pcs.get_evaluations_on_domain(data_t, 0, log_n + lqd)
        chunks = air.quotient(lde, log_n, pcs.params.log_blowup, pis, alpha)
        root_q, data_q = pcs.commit(list(zip(chunks, chunk_shifts(log_n, lqd))))
        ch.observe_digest(root_q)
        zeta = ch.sample_ext()
        g_n = from_monty(two_adic_generator(log_n))
        zeta_next = _monty([v * g_n for v in _canon(zeta)])
        opened, fri = pcs.open([(data_t, [[zeta, zeta_next]]), (data_q, [[zeta]] * len(chunks))], ch)
    finally:
        data_t.free()
        if data_q is not None:
            data_q.free()
        ch.free()
    u = lambda *v: np.array(v, dtype=np.uint32)
    o = opened.reshape(-1)
    head = [u(PROOF_MAGIC, 1, log_n), root_t, root_q, u(w), o[:4 * w], u(w), o[4 * w:8 * w], u(len(chunks))]
    for c in range(len(chunks)):
        head += [u(4), o[8 * w + 16 * c:8 * w + 16 * (c + 1)]]
    return np.concatenate(head).astype(np.uint32).tobytes() + fri


class AirProver:
    """p3_uni_stark::prove for ONE (air, log_n, params, hash, profile) in one device-resident launch chain (include/p3hip.h
    p3hip_air_prover_*): the arena is allocated here, a proof allocates nothing, keeps the transcript on the device and synchronises
    once.  The bytes are prove_air's.  The air may be freed once the prover exists.  own_stream=False: the launches go to the torch
    stream that is current NOW; True: to a stream the prover creates (two provers then overlap)."""

    def __init__(self, air, log_n, params=None, hash="poseidon2", profile="latency", own_stream=False):
        if not isinstance(air, Air) or not air._h:
            raise TypeError("AirProver: air must be a live Air")
        if not isinstance(log_n, (int, np.integer)) or isinstance(log_n, bool) or log_n < 1:
            raise ValueError("AirProver: log_n must be an integer >= 1")
        self.params = params or FriParameters()
        kind, prof = _hash_kind(hash), profile_kind(profile)
        self.log_n, self.hash, self.profile = int(log_n), hash, profile
        self.width, self.n_public = air.width, air.n_public
        self._h, self._own = C.c_void_p(), bool(own_stream)
        stream = None if own_stream else _stream_ptr()
        self._stream = None if own_stream else stream.value
        _lib.check(_lib.lib().p3hip_air_prover_create(air._h, prof, kind, self.log_n, C.cast(self.params._c(), C.c_void_p), stream,
                                                      1 if own_stream else 0, C.byref(self._h)))

    def _args(self, trace, pis):
        """-> (the trace as a contiguous numpy array or a device pointer, is it host memory, the public values); raises before any
        library call"""
        rows = 1 << self.log_n
        what = "AirProver: a (%d, %d) trace of 32-bit Montgomery words" % (rows, self.width)
        p = _words(pis if pis is not None else [], self.n_public)
        if _is_torch(trace):
            if tuple(trace.shape) != (rows, self.width) or trace.element_size() != 4 or trace.is_floating_point():
                raise ValueError(what + ", got %s %s" % (tuple(trace.shape), trace.dtype))
            if not trace.is_cuda or not trace.is_contiguous():
                raise ValueError("AirProver: the trace must be a contiguous device tensor")
            return trace, False, p
        host = np.ascontiguousarray(trace, dtype=np.uint32)
        if host.shape != (rows, self.width):
            raise ValueError(what + ", got %s" % (host.shape,))
        return host, True, p

    def _behind_torch(self):
        """the prover reads the tensor on ITS stream: what torch queued elsewhere to write it must be complete"""
        import torch
        cur = torch.cuda.current_stream()
        if self._own or cur.cuda_stream != self._stream:
            cur.synchronize()

    def prove(self, trace, pis=None, check_constraints=False):
        """trace: a (2^log_n, width) torch device tensor (read in place, left unchanged) or numpy array (uploaded); pis: n_public
        Montgomery words.  check_constraints=True runs Air.check_trace's pass first (one more synchronisation) and raises P3HipError
        naming the row and constraint; without it any trace is proven and the verifiers reject what does not hold."""
        t, host, p = self._args(trace, pis)
        if not self._h:
            raise ValueError("AirProver: closed")
        out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        pp = p.ctypes.data_as(C.c_void_p) if p.size else None
        flags = 1 if check_constraints else 0  # P3HIP_PROVE_CHECK_TRACE
        if host:
            _lib.check(_lib.lib().p3hip_air_prover_prove(self._h, t.ctypes.data_as(C.c_void_p), pp, flags, C.byref(out), C.byref(n)))
        else:
            self._behind_torch()
            _lib.check(_lib.lib().p3hip_air_prover_prove_dev(self._h, C.c_void_p(t.data_ptr()), pp, flags, C.byref(out), C.byref(n)))
        return C.string_at(out, n.value)

    def enqueue(self, trace, pis=None):
        """Queues the proof of a DEVICE trace and returns at once; one proof in flight.  Keep `trace` alive and unchanged until finish()."""
        t, host, p = self._args(trace, pis)
        if host:
            raise TypeError("AirProver.enqueue: a torch device tensor (prove() uploads numpy arrays)")
        if not self._h:
            raise ValueError("AirProver: closed")
        self._behind_torch()
        _lib.check(_lib.lib().p3hip_air_prover_enqueue_dev(self._h, C.c_void_p(t.data_ptr()), p.ctypes.data_as(C.c_void_p) if p.size else None))
        self._keep = t

    def finish(self):
        """Waits for the enqueued proof and returns its bytes."""
        if not self._h:
            raise ValueError("AirProver: closed")
        out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        try:
            _lib.check(_lib.lib().p3hip_air_prover_finish(self._h, C.byref(out), C.byref(n)))
        finally:
            self._keep = None
        return C.string_at(out, n.value)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().p3hip_air_prover_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AirRejected(_lib.P3HipError):
    """verify_air refused the proof: .code 1 magic / version, 2 log_n, 3 a count that is not the AIR's, 4 truncated or a word that is
    no field element, 10 OodEvaluationMismatch, or the PCS verifier's code (include/p3hip.h p3hip_pcs_verify)."""


def verify_air(air, proof, pis, log_n, params, hash="poseidon2"):
    """p3_uni_stark::verify for a proof of prove_air, host code.  Every count in the header is compared with the AIR's own; none is
    followed.  Returns None on accept, raises AirRejected otherwise."""
    from . import pcs as _pcs
    pis = _words(pis if pis is not None else [], air.n_public)
    w, lqd = air.width, air.log_quotient_degree
    if not isinstance(log_n, (int, np.integer)) or not 1 <= log_n <= 27 - lqd:
        raise ValueError("verify_air: log_n must lie in 1..%d for this AIR (the quotient domain has 2^(log_n + %d) points)" % (27 - lqd, lqd))
    n_chunks = 1 << lqd
    words = np.frombuffer(bytes(proof[:len(proof) // 4 * 4]), dtype=np.uint32)
    head_len = 3 + 16 + (1 + 4 * w) * 2 + 1 + 17 * n_chunks
    pos, bad = [0], [False]

    def u32():  # past the end: no count and no version is -1
        pos[0] += 1
        if pos[0] > len(words):
            bad[0] = True
            return -1
        return int(words[pos[0] - 1])

    def take(n):
        out = np.zeros(n, dtype=np.uint32)
        got = words[pos[0]:pos[0] + n]
        out[:len(got)] = got
        bad[0] |= len(got) < n
        pos[0] += n
        return out

    def reject(code, msg):
        raise AirRejected(code, msg)

    if u32() != PROOF_MAGIC or u32() != 1:
        reject(1, "bad magic or version")
    if u32() != log_n:
        reject(2, "log_n differs")
    root_t, root_q = take(8), take(8)
    if u32() != w:
        reject(3, "local values: the count is not the AIR's width")
    local = take(4 * w)
    if u32() != w:
        reject(3, "next values: the count is not the AIR's width")
    nxt = take(4 * w)
    if u32() != n_chunks:
        reject(3, "quotient chunks: the count is not the AIR's")
    chunks = []
    for c in range(n_chunks):
        if u32() != 4:
            reject(3, "quotient chunk %d: the width is not 4" % c)
        chunks.append(take(16))
    if bad[0]:
        reject(4, "truncated header")
    opened = np.concatenate([local, nxt] + chunks)
    if np.any(opened >= P) or (hash == "poseidon2" and (np.any(root_t >= P) or np.any(root_q >= P))):
        reject(4, "a header word is not a canonical field element")
    ch = Challenger(hash)
    alpha = _prefix(ch, log_n, root_t, pis)
    ch.observe_digest(root_q)
    zeta = ch.sample_ext()
    z = _canon(zeta)
    n = 1 << log_n
    g_n = from_monty(two_adic_generator(log_n))
    ginv = pow(g_n, P - 2, P)
    zeta_next = _monty([v * g_n for v in z])
    # selectors_at_point on the trace domain
    zh = _esub(_epow(z, n), _base(1))
    first = _emul(zh, _einv(_esub(z, _base(1))))
    last = _emul(zh, _einv(_esub(z, _base(ginv))))
    trans = _esub(z, _base(ginv))
    sels = np.concatenate([_monty(first), _monty(last), _monty(trans)])
    folded = _canon(air.eval_ext(local, nxt, pis, sels, alpha))
    # quotient(zeta) = sum_c zps_c sum_e X^e chunk_c[e], zps_c = prod_{j != c} Z_{D_j}(zeta) / Z_{D_j}(s_c), D_j = s_j <g_n>
    shifts = [from_monty(s) for s in chunk_shifts(log_n, lqd)]
    zn = _epow(z, n)
    quot = [0, 0, 0, 0]
    for c in range(n_chunks):
        zps = _base(1)
        for j in range(n_chunks):
            if j != c:
                sjn_inv = pow(pow(shifts[j], n, P), P - 2, P)
                num = _esub([v * sjn_inv % P for v in zn], _base(1))  # Z_{D_j}(x) = (x / s_j)^n - 1
                den = (pow(shifts[c], n, P) * sjn_inv - 1) % P
                zps = _emul(zps, [v * pow(den, P - 2, P) % P for v in num])
        ck = _canon(chunks[c])
        val = [0, 0, 0, 0]
        for e in range(4):
            be = [0, 0, 0, 0]
            be[e] = 1
            val = _eadd(val, _emul(be, ck[4 * e:4 * e + 4]))
        quot = _eadd(quot, _emul(zps, val))
    if folded != _emul(quot, zh):
        reject(OOD_EVALUATION_MISMATCH, "OodEvaluationMismatch")
    rounds = [((root_t, [w]), [[zeta, zeta_next]]), ((root_q, [4] * n_chunks), [[zeta]] * n_chunks)]
    try:
        _pcs.verify(params, hash, rounds, log_n, opened.reshape(-1, 4), bytes(proof[4 * head_len:]), ch)
    except PcsRejected as e:
        raise AirRejected(e.code, e.message)
    finally:
        ch.free()


# ---- the library's verifiers: one proof on the host (Air.verify), batches on the device ----
def air_proof_len(air, log_n, params, hash="poseidon2"):
    """The byte length every prove_air proof of `air` at 2^log_n rows has (p3hip_air_proof_len; host only).  A refused gate raises
    P3HipError(-1) naming it."""
    out = C.c_size_t()
    _lib.check(_lib.lib().p3hip_air_proof_len(air._h, _hash_kind(hash), int(log_n), C.cast(params._c(), C.c_void_p), C.byref(out)))
    return out.value


class AirVerifier:
    """p3_uni_stark::verify for batches of prove_air proofs of ONE (air, log_n, params, hash) on the device (include/p3hip.h
    p3hip_air_verifier_*).  The air may be freed once the verifier exists.  Statuses: 0 = accept, 10 OodEvaluationMismatch, the PCS
    verifier's 11 / 13 / 14 / 15, or VERIFY_MALFORMED (16)."""

    def __init__(self, air, log_n, params=None, hash="poseidon2", max_proofs=64):
        self.params = params or FriParameters()
        self.log_n, self.hash, self.max_proofs, self.n_public = int(log_n), hash, max_proofs, air.n_public
        self._h = C.c_void_p()
        _lib.check(_lib.lib().p3hip_air_verifier_create(air._h, _hash_kind(hash), self.log_n, C.cast(self.params._c(), C.c_void_p), max_proofs,
                                                        C.byref(self._h)))
        self.proof_len = air_proof_len(air, log_n, self.params, hash)

    def verify_many(self, proofs, pis):
        """proofs: a list of bytes; pis: (n, n_public) Montgomery words (None or empty when the AIR has no public values).  Returns a
        numpy uint32 array of statuses; batches larger than max_proofs are split."""
        n = len(proofs)
        status = np.zeros(n, dtype=np.uint32)
        if n == 0:
            return status
        p = _words(pis if pis is not None else [], n * self.n_public)
        ptrs = (C.c_char_p * n)(*[bytes(x) for x in proofs])
        lens = (C.c_size_t * n)(*[len(x) for x in proofs])
        _lib.check(_lib.lib().p3hip_air_verifier_verify(self._h, n, ptrs, lens, p.ctypes.data_as(C.c_void_p) if p.size else None,
                                                        status.ctypes.data_as(_lib.u32p)))
        return status

    def verify_many_dev(self, proofs, pis, lens=None, n=None, stride=None, status=None, rejected=None):
        """The device entry on torch tensors, enqueued on torch's current stream and not synchronised.  proofs: a contiguous uint8 /
        int32 device tensor, proof i at byte i * stride (default: the row length of a 2-d tensor); pis: a contiguous 32-bit device
        tensor of n x n_public words (None when the AIR has no public values); lens: n 32-bit byte lengths or None.  Returns (status,
        rejected): int32 device tensors of n codes and one count (rejected=False: no count is written, None is returned)."""
        import torch
        if n is None:
            n = proofs.shape[0] if proofs.dim() == 2 else (pis.numel() // self.n_public if self.n_public else 0)
        if stride is None:
            stride = proofs.stride(0) * proofs.element_size() if proofs.dim() == 2 else self.proof_len
        for t, words in ([(pis, n * self.n_public)] if self.n_public else []) + ([(lens, n)] if lens is not None else []):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != 4 or t.numel() < words:
                raise ValueError("expected contiguous device tensors of 32-bit words, one row per member")
        if not proofs.is_cuda or not proofs.is_contiguous():
            raise ValueError("expected contiguous device tensors")
        if n and proofs.numel() * proofs.element_size() < (n - 1) * stride + self.proof_len:
            raise ValueError("the proofs tensor is shorter than n proofs")
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.int32, device=proofs.device)
        if rejected is None:
            rejected = torch.empty(1, dtype=torch.int32, device=proofs.device)
        _lib.check(_lib.lib().p3hip_air_verifier_verify_dev(
            self._h, C.c_void_p(proofs.data_ptr()), stride, C.c_void_p(lens.data_ptr()) if lens is not None else None,
            C.c_void_p(pis.data_ptr()) if self.n_public else None, n, C.c_void_p(status.data_ptr()),
            C.c_void_p(rejected.data_ptr()) if rejected is not False else None, _stream_ptr()))
        return status[:n], (rejected if rejected is not False else None)

    def close(self):
        if self._h:
            _lib.lib().p3hip_air_verifier_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
