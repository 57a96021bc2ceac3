"""Host-side mirror of Plonky3's Pcs contract for TwoAdicFriPcs<BabyBear, GpuDft, MerkleTreeMmcs, ExtensionMmcs> over
caller-supplied matrices (include/p3hip.h "TwoAdicFriPcs over CALLER-SUPPLIED matrices"), and of the challengers a caller
drives between its calls; HidingFriPcs mirrors the hiding PCS the reference builds ("HidingFriPcs over CALLER-SUPPLIED matrices").
Every matrix of one open / verify has the same height, unless the object was created with mixed_heights=True (include/p3hip.h
p3hip_pcs_create_mixed; verify then takes a log height per matrix).  commit / open keep everything device-resident (one
synchronisation each); verify is host code of the library."""
import ctypes as C

import numpy as np

from . import _lib
from .fib_air import FriParameters, _hash_kind, profile_kind
from .gpu_dft import MONTY_ONE, P, _is_torch, _stream_ptr, dev_u32

MAX_MATS, MAX_ROUNDS, MAX_POINTS, MAX_COLS = 8, 4, 4, 8192  # csrc/prover.h PCS_MAX_*
HIDING_MAX_MATS, SALT, MAX_RANDOM_CODEWORDS, MAX_QUOTIENT_WIDTH = 4, 4, 8, 2048  # csrc/prover.h PCS_HIDING_MAX_MATS ...
STATE_WORDS = 128  # include/p3hip.h P3HIP_CHALLENGER_STATE_WORDS
MAX_SLOTS = 4  # csrc/pcs_verifier_dev.h PCS_MAX_SLOTS
# diagnostic, not a stable interface (a tuning detail that moves with measurements; the tests use it to run both forms)
WAVE_FORM_MIN_COLUMNS = 256  # csrc/pcs_verifier_dev.hip PV_WAVE_MIN_COLS: row words per query from which one wavefront serves a query


def _words(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    if n is not None and a.size != n:
        raise ValueError("expected %d words, got %d" % (n, a.size))
    return a


class PcsRejected(_lib.P3HipError):
    """verify refused the proof: .code is the failed check (include/p3hip.h p3hip_pcs_verify)."""


class Challenger:
    """DuplexChallenger<BabyBear, Poseidon2-16, 16, 8> (hash="poseidon2") or SerializingChallenger32 over a Keccak-256
    HashChallenger (hash="keccak") on the host.  Field elements are Montgomery words."""

    def __init__(self, hash="poseidon2", _handle=None):
        self.hash = hash
        self._h = _handle
        if _handle is None:
            self._h = C.c_void_p()
            _lib.check(_lib.lib().p3hip_challenger_create(_hash_kind(hash), C.byref(self._h)))

    def observe(self, words):
        w = _words(words)
        _lib.check(_lib.lib().p3hip_challenger_observe(self._h, w.ctypes.data_as(C.c_void_p), w.size))

    def observe_digest(self, digest):
        d = _words(digest, 8)
        _lib.check(_lib.lib().p3hip_challenger_observe_digest(self._h, d.ctypes.data_as(C.c_void_p)))

    def sample_ext(self):
        out = np.zeros(4, dtype=np.uint32)
        _lib.check(_lib.lib().p3hip_challenger_sample_ext(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def sample_bits(self, bits):
        out = C.c_uint32()
        _lib.check(_lib.lib().p3hip_challenger_sample_bits(self._h, bits, C.byref(out)))
        return out.value

    def clone(self):
        h = C.c_void_p()
        _lib.check(_lib.lib().p3hip_challenger_clone(self._h, C.byref(h)))
        return Challenger(self.hash, h)

    def export_state(self):
        """The challenger as the STATE_WORDS words a device transcript imports (include/p3hip.h p3hip_challenger_export)."""
        out = np.zeros(STATE_WORDS, dtype=np.uint32)
        _lib.check(_lib.lib().p3hip_challenger_export(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def import_state(self, words):
        """The inverse of export_state; counters no challenger can hold are refused (P3HipError -1, the challenger unchanged)."""
        w = _words(words, STATE_WORDS)
        _lib.check(_lib.lib().p3hip_challenger_import(self._h, w.ctypes.data_as(C.c_void_p)))

    def free(self):
        if self._h:
            _lib.lib().p3hip_challenger_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PcsProverData:
    """Prover data of one commitment: the bit-reversed LDEs in HBM and their Merkle tree."""

    def __init__(self, handle, root, dims, keep):
        self._h, self.root, self.dims, self._keep = handle, root, dims, keep  # dims: (height, width) of the committed evaluations

    def free(self):
        if self._h:
            _lib.lib().p3hip_pcs_data_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _flatten(rounds):
    """rounds = [(x, [points of matrix 0, points of matrix 1, ...])] -> per-matrix point counts and the points' words, round ->
    matrix -> point."""
    counts, pts = [], []
    for _, mat_points in rounds:
        for ps in mat_points:
            counts.append(len(ps))
            pts += [_words(z, 4) for z in ps]
    points = np.concatenate(pts) if pts else np.zeros(4, dtype=np.uint32)
    return (C.c_size_t * max(len(counts), 1))(*counts), points, counts


class TwoAdicFriPcs:
    _hiding = False

    def __init__(self, params=None, hash="poseidon2", profile="latency", own_stream=False, mixed_heights=False):
        """mixed_heights: commit and open take matrices of any power-of-two heights (p3hip_pcs_create_mixed); False: they refuse
        them by name.  A same-height open is the same either way."""
        import torch
        self.params = params or FriParameters()
        self.hash, self._kind = hash, _hash_kind(hash)
        self.mixed_heights = bool(mixed_heights)
        self._h = C.c_void_p()
        torch.cuda.current_stream()  # make sure a context exists
        create = _lib.lib().p3hip_pcs_create_mixed if mixed_heights else _lib.lib().p3hip_pcs_create
        _lib.check(create(profile_kind(profile), self._kind, C.cast(self.params._c(), C.c_void_p),
                          None if own_stream else _stream_ptr(), 1 if own_stream else 0, C.byref(self._h)))

    def commit(self, evaluations):
        """Pcs::commit.  evaluations: [(matrix, domain shift)] — the matrix a (h, w) torch device tensor (read in place) or numpy
        array (uploaded) of evaluations over shift * <g_h> in natural row order; shift a Montgomery word (None: 1).  Returns
        (root as numpy uint32[8], PcsProverData)."""
        L = _lib.lib()
        mats = [m.contiguous() if _is_torch(m) else dev_u32(m) for m, _ in evaluations]
        for m in mats:
            if m.dim() != 2 or m.element_size() != 4 or not m.is_cuda:
                raise ValueError("commit: (h, w) device matrices of 32-bit words")
        n = len(mats)
        ptrs = (C.c_void_p * max(n, 1))(*[m.data_ptr() for m in mats])
        hs = (C.c_size_t * max(n, 1))(*[m.shape[0] for m in mats])
        ws = (C.c_size_t * max(n, 1))(*[m.shape[1] for m in mats])
        shifts = np.array([MONTY_ONE if s is None else int(s) for _, s in evaluations], dtype=np.uint32)
        root = np.zeros(8, dtype=np.uint32)
        h = C.c_void_p()
        _lib.check(L.p3hip_pcs_commit_dev(self._h, ptrs, hs, ws, shifts.ctypes.data_as(C.c_void_p), n, root.ctypes.data_as(C.c_void_p),
                                          C.byref(h)))
        return root, PcsProverData(h, root, [tuple(m.shape) for m in mats], mats)

    def get_evaluations_on_domain(self, data, i, log_size):
        """Pcs::get_evaluations_on_domain for the disjoint coset GENERATOR * <g_(2^log_size)>: a torch VIEW of the stored LDE's first
        2^log_size rows (no copy); natural index k sits at row bitrev(k, log_size)."""
        import torch
        p, hh, ww = C.c_void_p(), C.c_size_t(), C.c_size_t()
        _lib.check(_lib.lib().p3hip_pcs_lde_dev(data._h, i, C.byref(p), C.byref(hh), C.byref(ww)))
        m = 1 << log_size
        if m < data.dims[i][0] or m > hh.value:  # hh: the matrix's own LDE height
            raise ValueError("get_evaluations_on_domain: 2^log_size must lie between the matrix height and the LDE height")

        class _View:  # the CUDA array interface: torch wraps the memory without copying; `owner` keeps the LDE alive
            def __init__(self, owner):
                self.owner = owner
                self.__cuda_array_interface__ = {"shape": (m, ww.value), "typestr": "<i4", "data": (p.value, False), "version": 2}
        return torch.as_tensor(_View(data), device="cuda")

    def open(self, rounds, challenger):
        """Pcs::open.  rounds = [(PcsProverData, [points of matrix 0, ...])], a point = 4 Montgomery words.  The challenger is
        advanced to the state after the last query index.  Returns (opened values as numpy uint32 (n, 4) in observation order
        round -> matrix -> point -> column, proof bytes: the FriProof section of the wire format)."""
        L = _lib.lib()
        n = len(rounds)
        for d, mp in rounds:
            if len(mp) != len(d.dims):
                raise ValueError("open: one list of points per committed matrix")
        handles = (C.c_void_p * max(n, 1))(*[d._h for d, _ in rounds])
        counts, points, cl = _flatten(rounds)
        total = sum(len(ps) * d.dims[i][1] for d, mp in rounds for i, ps in enumerate(mp))
        opened = np.zeros((max(total, 1), 4), dtype=np.uint32)
        out, ln = C.POINTER(C.c_uint8)(), C.c_size_t()
        _lib.check(L.p3hip_pcs_open(self._h, handles, n, counts, points.ctypes.data_as(C.c_void_p), challenger._h,
                                    opened.ctypes.data_as(C.c_void_p), opened.size, C.byref(out), C.byref(ln)))
        return opened[:total], C.string_at(out, ln.value)

    def verify(self, rounds, log_h, opened, proof, challenger):
        """Pcs::verify (see verify)."""
        return verify(self.params, self.hash, rounds, log_h, opened, proof, challenger, hiding=self._hiding)

    def free(self):
        if self._h:
            _lib.lib().p3hip_pcs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HidingFriPcs(TwoAdicFriPcs):
    """HidingFriPcs::new(dft, mmcs, fri_params, num_random_codewords, SmallRng::seed_from_u64(pcs_seed)) over a MerkleTreeHidingMmcs
    seeded with mmcs_seed (native/src/fib_air.rs:40-65: 4, 1, 1).  The object owns the three random streams, which advance from call
    to call.  commit (inherited) randomizes: the prover data's dims are those of the committed matrices, (2h, w +
    num_random_codewords), and get_evaluations_on_domain returns all of those columns, the caller's own first."""
    _hiding = True

    def __init__(self, params=None, hash="poseidon2", profile="latency", num_random_codewords=4, mmcs_seed=1, pcs_seed=1, own_stream=False):
        import torch
        self.params = params or FriParameters()
        self.hash, self._kind = hash, _hash_kind(hash)
        self.num_random_codewords = num_random_codewords
        self._h = C.c_void_p()
        torch.cuda.current_stream()  # make sure a context exists
        _lib.check(_lib.lib().p3hip_pcs_create_hiding(profile_kind(profile), self._kind, C.cast(self.params._c(), C.c_void_p),
                                                      num_random_codewords, mmcs_seed, pcs_seed, None if own_stream else _stream_ptr(),
                                                      1 if own_stream else 0, C.byref(self._h)))

    def commit(self, evaluations):
        """HidingFriPcs::commit: as TwoAdicFriPcs.commit, at most 4 matrices."""
        root, data = super().commit(evaluations)
        data.dims = [(2 * h, w + self.num_random_codewords) for h, w in data.dims]
        return root, data

    def commit_quotient(self, chunks):
        """HidingFriPcs::commit_quotient.  chunks: 2 or 4 (h, w) matrices, chunk c the evaluations in natural order on the coset
        GENERATOR * g_(len(chunks) h)^c * <g_h>.  Returns (root, PcsProverData) of the blinded chunk matrices, (2h, w) each."""
        mats = [m.contiguous() if _is_torch(m) else dev_u32(m) for m in chunks]
        for m in mats:
            if m.dim() != 2 or m.element_size() != 4 or not m.is_cuda or m.shape != mats[0].shape:
                raise ValueError("commit_quotient: (h, w) device matrices of 32-bit words, all of one shape")
        n = len(mats)
        h, w = (int(v) for v in mats[0].shape) if n else (0, 0)
        ptrs = (C.c_void_p * max(n, 1))(*[m.data_ptr() for m in mats])
        root, hd = np.zeros(8, dtype=np.uint32), C.c_void_p()
        _lib.check(_lib.lib().p3hip_pcs_commit_quotient_dev(self._h, ptrs, h, w, n, root.ctypes.data_as(C.c_void_p), C.byref(hd)))
        return root, PcsProverData(hd, root, [(2 * h, w)] * n, mats)

    def get_opt_randomization_poly_commitment(self, log_h):
        """HidingFriPcs::get_opt_randomization_poly_commitment for traces of 2^log_h rows -> (root, PcsProverData) of the (2h,
        num_random_codewords + 4) random matrix."""
        root, hd = np.zeros(8, dtype=np.uint32), C.c_void_p()
        _lib.check(_lib.lib().p3hip_pcs_commit_randomization(self._h, log_h, root.ctypes.data_as(C.c_void_p), C.byref(hd)))
        return root, PcsProverData(hd, root, [(2 << log_h, self.num_random_codewords + 4)], [])


def verify(params, hash, rounds, log_h, opened, proof, challenger, hiding=False):
    """Pcs::verify on the host.  rounds = [((root, [width of matrix 0, ...]), [points of matrix 0, ...])]; opened as open returns
    it.  Returns None on accept; raises PcsRejected (code = the failed check) on a rejection and P3HipError(-1) for a refused
    argument.  The challenger is advanced as the verifier advances it.  hiding: HidingFriPcs::verify — log_h the caller's log
    height, the widths the committed ones.  log_h: an int (every matrix of that height: p3hip_pcs_verify), or per-matrix lists
    [[log height of matrix 0, ...] per round] (mixed heights: p3hip_pcs_verify_mixed; not with hiding)."""
    L = _lib.lib()
    mixed = not isinstance(log_h, (int, np.integer))
    if mixed:
        if hiding:
            raise ValueError("verify: a hiding PCS takes one log height, not per-matrix lists")
        lhs = [int(v) for r in log_h for v in r]
        if [len(r) for r in log_h] != [len(ws) for (_, ws), _ in rounds]:
            raise ValueError("verify: one log height per matrix")
        log_h = (C.c_uint * max(len(lhs), 1))(*lhs)
    n = len(rounds)
    roots = np.concatenate([_words(r, 8) for (r, _), _ in rounds]) if n else np.zeros(8, np.uint32)
    mats = [len(ws) for (_, ws), _ in rounds]
    widths = [int(w) for (_, ws), _ in rounds for w in ws]
    for (_, ws), mp in rounds:
        if len(mp) != len(ws):
            raise ValueError("verify: one list of points per matrix")
    counts, points, _ = _flatten(rounds)
    opened = _words(opened, 4 * sum(len(ps) * int(ws[i]) for (_, ws), mp in rounds for i, ps in enumerate(mp)))
    buf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(bytes(proof) or b"\0")
    code = C.c_int()
    fn = L.p3hip_pcs_verify_hiding if hiding else L.p3hip_pcs_verify_mixed if mixed else L.p3hip_pcs_verify
    _lib.check(fn(
        _hash_kind(hash), C.cast(params._c(), C.c_void_p), log_h, roots.ctypes.data_as(C.c_void_p), (C.c_size_t * max(n, 1))(*mats), (C.c_size_t * max(len(widths), 1))(*widths), n, counts, points.ctypes.data_as(C.c_void_p),
        opened.ctypes.data_as(C.c_void_p), buf, len(proof), challenger._h, C.byref(code)))
    if code.value:
        raise PcsRejected(code.value, _lib.take_last_error() or "")


class _Shape(C.Structure):
    _fields_ = [("log_h", C.c_uint), ("n_rounds", C.c_size_t), ("mats_per_round", C.POINTER(C.c_size_t)), ("widths", C.POINTER(C.c_size_t)),
                ("points_per_mat", C.POINTER(C.c_size_t)), ("n_slots", C.c_size_t), ("slots", C.POINTER(C.c_uint32))]


def _shape(log_h, rounds, n_slots):
    """rounds = [[(width, [slot of point 0, ...]) per matrix] per round] -> (p3hip_pcs_shape_t, what it points to)."""
    mats = [len(r) for r in rounds]
    widths = [int(w) for r in rounds for w, _ in r]
    counts = [len(sl) for r in rounds for _, sl in r]
    slots = [int(x) for r in rounds for _, sl in r for x in sl]
    keep = ((C.c_size_t * max(len(mats), 1))(*mats), (C.c_size_t * max(len(widths), 1))(*widths),
            (C.c_size_t * max(len(counts), 1))(*counts), (C.c_uint32 * max(len(slots), 1))(*slots))
    return _Shape(log_h, len(rounds), keep[0], keep[1], keep[2], n_slots, keep[3]), keep


def _log_heights(log_h, rounds, hiding, who):
    """log_h as PcsVerifier / pcs_proof_len take it -> None for an int (every matrix of that height), or the per-matrix lists
    [[log height per matrix] per round] flattened for the mixed entries (include/p3hip.h p3hip_pcs_verifier_create_mixed)"""
    if not isinstance(log_h, (list, tuple)):  # anything else goes down the same-height path, which says what it makes of it
        return None
    if hiding:
        raise ValueError("%s: a hiding PCS takes one log height, not per-matrix lists" % who)
    if [len(r) for r in log_h] != [len(r) for r in rounds]:
        raise ValueError("%s: one log height per matrix" % who)
    lhs = [int(v) for r in log_h for v in r]
    return (C.c_uint * max(len(lhs), 1))(*lhs)


def pcs_proof_len(params, hash, log_h, rounds, n_slots, hiding=False):
    """The byte length every proof of the shape has (host only; log_h and rounds as PcsVerifier takes them)."""
    lhs = _log_heights(log_h, rounds, hiding, "pcs_proof_len")
    sh, _keep = _shape(0 if lhs is not None else log_h, rounds, n_slots)
    out = C.c_size_t()
    if lhs is not None:
        _lib.check(_lib.lib().p3hip_pcs_proof_len_mixed(_hash_kind(hash), 0, C.cast(params._c(), C.c_void_p), C.byref(sh), lhs, C.byref(out)))
    else:
        _lib.check(_lib.lib().p3hip_pcs_proof_len(_hash_kind(hash), 1 if hiding else 0, C.cast(params._c(), C.c_void_p), C.byref(sh), C.byref(out)))
    return out.value


class PcsVerifier:
    """Pcs::verify of TwoAdicFriPcs / HidingFriPcs for batches of members of ONE shape, on the device (include/p3hip.h "batches of PCS
    proofs verified ON THE DEVICE").  rounds = [[(committed width, [slot of point 0, ...]) per matrix] per round]; a member supplies
    n_slots points.  log_h: an int (every matrix of that height), or per-matrix lists [[log height per matrix] per round] as verify
    takes them (mixed heights: p3hip_pcs_verifier_create_mixed; ValueError with hiding).  Statuses: 0 = accept, the host verifier's
    codes 11 / 13 / 14 / 15, or VERIFY_MALFORMED (16)."""

    def __init__(self, log_h, rounds, n_slots, params=None, hash="poseidon2", hiding=False, max_proofs=64):
        self.params = params or FriParameters()
        self.log_h, self.rounds, self.n_slots, self.hash, self.hiding, self.max_proofs = log_h, rounds, n_slots, hash, hiding, max_proofs
        self.n_rounds = len(rounds)
        self.total = sum(int(w) * len(sl) for r in rounds for w, sl in r)
        self._h = C.c_void_p()
        lhs = _log_heights(log_h, rounds, hiding, "PcsVerifier")
        sh, _keep = _shape(0 if lhs is not None else log_h, rounds, n_slots)
        if lhs is not None:
            _lib.check(_lib.lib().p3hip_pcs_verifier_create_mixed(_hash_kind(hash), 0, C.cast(self.params._c(), C.c_void_p), C.byref(sh), lhs,
                                                                  max_proofs, C.byref(self._h)))
        else:
            _lib.check(_lib.lib().p3hip_pcs_verifier_create(_hash_kind(hash), 1 if hiding else 0, C.cast(self.params._c(), C.c_void_p), C.byref(sh),
                                                            max_proofs, C.byref(self._h)))
        self.proof_len = pcs_proof_len(self.params, hash, log_h, rounds, n_slots, hiding)
        self.wave_form = bool(_lib.lib().p3hip_pcs_verifier_wave_form(self._h))

    def verify_many(self, proofs, roots, points, opened, challengers):
        """proofs: a list of bytes; roots (n, n_rounds, 8), points (n, n_slots, 4), opened (n, total, 4): numpy uint32; challengers: a
        list of Challenger, each the member's transcript before verification — an accepted member's is advanced as the host
        verifier advances it, a rejected member's is left alone.  Returns a numpy uint32 array of statuses; batches larger than
        max_proofs are split."""
        n = len(proofs)
        status = np.zeros(n, dtype=np.uint32)
        if n == 0:
            return status
        if len(challengers) != n:
            raise ValueError("one challenger per proof")
        r, p, o = _words(roots, n * self.n_rounds * 8), _words(points, n * self.n_slots * 4), _words(opened, n * self.total * 4)
        ptrs = (C.c_char_p * n)(*[bytes(x) for x in proofs])
        lens = (C.c_size_t * n)(*[len(x) for x in proofs])
        ch = (C.c_void_p * n)(*[c._h for c in challengers])
        _lib.check(_lib.lib().p3hip_pcs_verifier_verify(self._h, n, ptrs, lens, r.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                                                        o.ctypes.data_as(C.c_void_p), ch, status.ctypes.data_as(_lib.u32p)))
        return status

    def verify_many_dev(self, proofs, roots, points, opened, chal_in, lens=None, n=None, stride=None, status=None, rejected=None,
                        chal_out=None):
        """The device entry on torch tensors, enqueued on torch's current stream and not synchronised.  proofs: a contiguous uint8 /
        int32 device tensor, proof i at byte i * stride (default: the row length of a 2-d tensor); roots, points, opened, chal_in:
        contiguous 32-bit device tensors of n x n_rounds x 8, n x n_slots x 4, n x total x 4 and n x STATE_WORDS words; lens: n 32-bit
        byte lengths or None.  Returns (status, rejected, chal_out): int32 device tensors of n codes, one count and n x STATE_WORDS
        words (chal_out=False: no transcripts are written, None is returned)."""
        import torch
        if n is None:
            n = chal_in.shape[0]
        if stride is None:
            stride = proofs.stride(0) * proofs.element_size() if proofs.dim() == 2 else self.proof_len
        need = ((roots, n * self.n_rounds * 8), (points, n * self.n_slots * 4), (opened, n * self.total * 4), (chal_in, n * STATE_WORDS))
        for t, words in need + (((lens, n),) if lens is not None else ()):
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
        if chal_out is None:
            chal_out = torch.empty((max(n, 1), STATE_WORDS), dtype=torch.int32, device=proofs.device)
        _lib.check(_lib.lib().p3hip_pcs_verifier_verify_dev(
            self._h, C.c_void_p(proofs.data_ptr()), stride, C.c_void_p(lens.data_ptr()) if lens is not None else None,
            C.c_void_p(roots.data_ptr()), C.c_void_p(points.data_ptr()), C.c_void_p(opened.data_ptr()), C.c_void_p(chal_in.data_ptr()), n,
            C.c_void_p(status.data_ptr()), C.c_void_p(rejected.data_ptr()), C.c_void_p(chal_out.data_ptr()) if chal_out is not False else None,
            _stream_ptr()))
        return status[:n], rejected, (chal_out[:n] if chal_out is not False else None)

    def close(self):
        if self._h:
            _lib.lib().p3hip_pcs_verifier_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
