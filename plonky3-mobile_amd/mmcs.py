"""Host-side mirror of Plonky3's Mmcs contract: MerkleTreeMmcs over either hash configuration —
"poseidon2" (north_star: Poseidon2 sponge 16/8/8 + TruncatedPermutation, digest 8 field elements) or "keccak"
(what the reference itself wires at native/src/fib_air.rs:28-51: PaddingFreeSponge<KeccakF,25,17,4> behind
SerializingHasher + CompressionFunctionFromHasher, digest [u64;4]), plain or hiding.  All four methods are here: commit /
open_batch / get_matrices keep everything device-resident; verify_batch is host code of the library (p3hip_mmcs_verify_batch: what
the proof verifiers run on their openings); open_batch_many / verify_batch_many open and verify n indices of one commitment in one
launch each, device to device."""
import ctypes as C

import numpy as np

from . import _lib
from .gpu_dft import _is_torch, _stream_ptr, dev_u32


def poseidon2_permute(states):
    """n x 16 states (torch device tensor in place, or numpy -> new array)."""
    L = _lib.lib()
    if _is_torch(states):
        assert states.is_cuda and states.is_contiguous() and states.shape[-1] == 16
        _lib.check(L.p3hip_poseidon2_permute_dev(C.c_void_p(states.data_ptr()), states.numel() // 16, _stream_ptr()))
        return states
    a = np.ascontiguousarray(states, dtype=np.uint32).copy()
    assert a.shape[-1] == 16
    _lib.check(L.p3hip_poseidon2_permute(a.ctypes.data_as(C.c_void_p), a.size // 16))
    return a


HASH_POSEIDON2, HASH_KECCAK = 0, 1


def keccak_f(states):
    """KeccakF::permute_mut on n x 25 u64 states (torch device int64 tensor in place, or numpy uint64 -> new array)."""
    import torch
    L = _lib.lib()
    if _is_torch(states):
        assert states.is_cuda and states.is_contiguous() and states.shape[-1] == 25 and states.element_size() == 8
        _lib.check(L.p3hip_keccak_f_dev(C.c_void_p(states.data_ptr()), states.numel() // 25, _stream_ptr()))
        return states
    a = np.ascontiguousarray(states, dtype=np.uint64)
    assert a.shape[-1] == 25
    d = torch.from_numpy(a.view(np.int64).copy()).cuda()
    _lib.check(L.p3hip_keccak_f_dev(C.c_void_p(d.data_ptr()), a.size // 25, _stream_ptr()))
    return d.cpu().numpy().view(np.uint64).reshape(a.shape)


def poseidon2_permute_variant(states, variant):
    """Test / diagnostics: one FORM of the permutation on a torch device tensor of n x 16 words, in place.  0 = int32 per lane, 1 = fp64
    per lane, 2 = fp64 per quad, 3 = int32 per 16-lane row (include/p3hip.h)."""
    assert _is_torch(states) and states.is_cuda and states.is_contiguous() and states.shape[-1] == 16 and states.element_size() == 4
    _lib.check(_lib.lib().p3hip_poseidon2_permute_variant_dev(C.c_void_p(states.data_ptr()), states.numel() // 16, variant, _stream_ptr()))
    return states


def keccak_f_variant(states, variant):
    """Test / diagnostics: one FORM of Keccak-f on a torch device int64 tensor of n x 25 words, in place.  0 = permute, 1 = permute_digest
    (words 0..3 written, the rest left as they were), 2 = f_coop (one state per wave)."""
    assert _is_torch(states) and states.is_cuda and states.is_contiguous() and states.shape[-1] == 25 and states.element_size() == 8
    _lib.check(_lib.lib().p3hip_keccak_f_variant_dev(C.c_void_p(states.data_ptr()), states.numel() // 25, variant, _stream_ptr()))
    return states


def compress_layer_variant(hash, variant, layer):
    """Test / diagnostics: one 2-to-1 compression layer through the production kernel of a named form.  layer: torch device tensor of
    2 n x 8 words; returns a new n x 8 tensor.  hash: "poseidon2" | "keccak"; variant as in include/p3hip.h."""
    import torch
    assert _is_torch(layer) and layer.is_cuda and layer.is_contiguous() and layer.shape[-1] == 8 and layer.element_size() == 4
    n_in = layer.numel() // 8
    assert n_in % 2 == 0
    out = torch.zeros((n_in // 2, 8), dtype=layer.dtype, device=layer.device)
    kind = {"poseidon2": HASH_POSEIDON2, "keccak": HASH_KECCAK}[hash]
    _lib.check(_lib.lib().p3hip_compress_layer_variant_dev(kind, variant, C.c_void_p(layer.data_ptr()), C.c_void_p(out.data_ptr()), n_in // 2,
                                                           _stream_ptr()))
    return out


class MerkleTree:
    """Prover data of one commitment: device digest layers + the committed matrices (kept alive)."""

    def __init__(self, handle, mats, root):
        self._h = handle
        self.mats = mats
        self.root = root
        self.log_max_height = _lib.lib().p3hip_mmcs_log_max_height(handle)

    def digest_layers(self):
        """All digest layers as numpy arrays (len, 8) — test/inspection helper (downloads)."""
        L = _lib.lib()
        out = []
        for l in range(L.p3hip_mmcs_num_layers(self._h)):
            n = C.c_size_t()
            p = L.p3hip_mmcs_layer_dev(self._h, l, C.byref(n))
            a = np.zeros((n.value, 8), dtype=np.uint32)
            _lib.check(L.p3hip_download(a.ctypes.data_as(C.c_void_p), C.c_void_p(p), a.nbytes))
            out.append(a)
        return out

    def free(self):
        if self._h:
            _lib.lib().p3hip_mmcs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MerkleTreeMmcs:
    def __init__(self, hash="poseidon2"):
        kinds = {"poseidon2": HASH_POSEIDON2, "keccak": HASH_KECCAK}
        if hash not in kinds:
            raise ValueError("unknown hash configuration %r" % (hash,))
        self.hash, self._kind = hash, kinds[hash]

    def commit(self, mats):
        """Mmcs::commit.  mats: list of 2-D matrices (torch device tensors stay resident; numpy arrays are
        uploaded).  Returns (root as numpy uint32[8], MerkleTree)."""
        import torch
        L = _lib.lib()
        dmats = [m.contiguous() if _is_torch(m) else dev_u32(m) for m in mats]
        n = len(dmats)
        ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in dmats])
        hs = (C.c_size_t * n)(*[m.shape[0] for m in dmats])
        ws = (C.c_size_t * n)(*[m.shape[1] for m in dmats])
        root = np.zeros(8, dtype=np.uint32)
        handle = C.c_void_p()
        torch.cuda.current_stream()  # make sure a context exists
        _lib.check(L.p3hip_mmcs_commit_hash_dev(self._kind, ptrs, hs, ws, n, root.ctypes.data_as(C.c_void_p),
                                                C.byref(handle), _stream_ptr()))
        return root, MerkleTree(handle, dmats, root)

    def commit_matrix(self, mat):
        return self.commit([mat])

    def get_matrices(self, tree):
        return tree.mats

    def get_max_height(self, tree):
        return 1 << tree.log_max_height

    def open_batch(self, index, tree):
        """Mmcs::open_batch -> (list of opened rows per matrix, sibling path (log_max_height, 8))."""
        tot = sum(m.shape[1] for m in tree.mats)
        rows = np.zeros(max(tot, 1), dtype=np.uint32)
        path = np.zeros((max(tree.log_max_height, 1), 8), dtype=np.uint32)
        _lib.check(_lib.lib().p3hip_mmcs_open_batch(tree._h, index, rows.ctypes.data_as(C.c_void_p),
                                                    path.ctypes.data_as(C.c_void_p), _stream_ptr()))
        out, off = [], 0
        for m in tree.mats:
            out.append(rows[off:off + m.shape[1]].copy())
            off += m.shape[1]
        return out, path[: tree.log_max_height].copy()


    # ---- Mmcs::verify_batch and the bulk, device-resident forms of both halves ----
    @staticmethod
    def _dims(dims):
        n = len(dims)
        return (C.c_size_t * n)(*[int(d[0]) for d in dims]), (C.c_size_t * n)(*[int(d[1]) for d in dims]), n

    def _verify(self, root, dims, index, rows, path):
        hs, ws, n = self._dims(dims)
        root = np.ascontiguousarray(root, dtype=np.uint32).reshape(-1)
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        path = np.ascontiguousarray(path, dtype=np.uint32).reshape(-1, 8)
        if root.size != 8 or rows.size != sum(int(d[1]) for d in dims):
            raise ValueError("verify_batch: the root has 8 words and the opened values one row per matrix of dims")
        rc = _lib.lib().p3hip_mmcs_verify_batch(self._kind, root.ctypes.data_as(C.c_void_p), hs, ws, n, int(index),
                                                rows.ctypes.data_as(C.c_void_p), path.ctypes.data_as(C.c_void_p), path.shape[0])
        if rc == 0:
            return True
        msg = _lib.take_last_error() or ""
        if rc == ROOT_MISMATCH:
            return False
        if rc > 0:
            raise ValueError(msg)
        raise _lib.P3HipError(rc, msg)

    def verify_batch(self, root, dims, index, opened_values, proof):
        """Mmcs::verify_batch: dims = [(height, width)] per matrix, opened_values = the opened row of every matrix, proof = the
        sibling path (log_max_height, 8).  True / False for accept / RootMismatch; the other rejects (wrong path length, a word
        that is no canonical field element, an index outside the tree) raise ValueError with the library's message."""
        rows = np.concatenate([np.asarray(v, dtype=np.uint32).reshape(-1) for v in opened_values]) if len(opened_values) else np.zeros(0, np.uint32)
        return self._verify(root, dims, index, rows, proof)

    def _open_many(self, indices, tree):
        import torch
        L = _lib.lib()
        idx = indices.contiguous() if _is_torch(indices) else dev_u32(np.asarray(indices, dtype=np.uint32).reshape(-1))
        assert idx.is_cuda and idx.element_size() == 4
        n, depth, rw = idx.numel(), tree.log_max_height, L.p3hip_mmcs_row_words(tree._h)
        rows = torch.empty((n, rw), dtype=torch.int32, device=idx.device)
        paths = torch.empty((n, depth, 8), dtype=torch.int32, device=idx.device)
        _lib.check(L.p3hip_mmcs_open_batch_many_dev(tree._h, C.c_void_p(idx.data_ptr()), n, C.c_void_p(rows.data_ptr()),
                                                    C.c_void_p(paths.data_ptr()), _stream_ptr()))
        return rows, paths

    def open_batch_many(self, indices, tree):
        """Mmcs::open_batch for n indices (a device int32 tensor, or anything numpy takes) in one launch -> device tensors
        rows [n, row_words] (matrix order) and paths [n, log_max_height, 8].  An index is masked into the tree."""
        return self._open_many(indices, tree)

    def _verify_many(self, root, dims, indices, rows, paths, form=0, with_rejected=False):
        import torch
        hs, ws, nm = self._dims(dims)
        root = np.ascontiguousarray(root, dtype=np.uint32).reshape(-1)
        assert root.size == 8
        idx = indices.contiguous() if _is_torch(indices) else dev_u32(np.asarray(indices, dtype=np.uint32).reshape(-1))
        rows, paths = rows.contiguous(), paths.contiguous()
        n, rw = idx.numel(), sum(int(d[1]) for d in dims)
        depth = max(int(d[0]) for d in dims).bit_length() - 1 if nm else 0
        if rows.numel() != n * rw or paths.numel() != n * depth * 8 or rows.element_size() != 4 or paths.element_size() != 4:
            raise ValueError("verify_batch_many: rows is [n, sum of the widths] and paths [n, log2 of the tallest height, 8], 32-bit words")
        status = torch.empty(n, dtype=torch.int32, device=idx.device)
        rejected = torch.empty(1, dtype=torch.int32, device=idx.device) if with_rejected else None  # the counter may be null
        _lib.check(_lib.lib().p3hip_mmcs_verify_batch_many_form_dev(
            int(form), self._kind, root.ctypes.data_as(C.c_void_p), hs, ws, nm, C.c_void_p(idx.data_ptr()), n, C.c_void_p(rows.data_ptr()),
            C.c_void_p(paths.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(rejected.data_ptr()) if with_rejected else None, _stream_ptr()))
        return (status, rejected) if with_rejected else status

    def verify_batch_many(self, root, dims, indices, rows, paths, form=0, with_rejected=False):
        """Mmcs::verify_batch for n openings of one commitment in one launch, in the layout open_batch_many returns -> a device
        tensor of n codes (0 = accept, ROOT_MISMATCH, NOT_CANONICAL, BAD_INDEX); with_rejected: also the device word counting the
        nonzero ones.  form: 0 = the library chooses by n, FORM_LANE / FORM_COOP force a kernel form (same codes)."""
        return self._verify_many(root, dims, indices, rows, paths, form, with_rejected)


ROOT_MISMATCH, WRONG_HEIGHT, NOT_CANONICAL, BAD_INDEX = 1, 2, 3, 4
FORM_AUTO, FORM_LANE, FORM_COOP = 0, 1, 2


class MerkleTreeHidingMmcs(MerkleTreeMmcs):
    """MerkleTreeHidingMmcs<.., SmallRng, .., SALT_ELEMS 4> (native/src/fib_air.rs:40-51): commit salts every matrix with
    draws from the MMCS's own rng (a DeviceRng: the stream lives in HBM); open_batch returns (values, (salts, siblings))."""
    SALT_ELEMS = 4

    def __init__(self, hash="keccak", rng=None, seed=1):
        super().__init__(hash)
        self._rng, self._seed = rng, seed

    @property
    def rng(self):
        """the MMCS's own rng, created on first use: verify_batch is host code and needs none"""
        if self._rng is None:
            from .fib_air import DeviceRng
            self._rng = DeviceRng(self._seed)
        return self._rng

    @rng.setter
    def rng(self, value):
        self._rng = value

    def commit(self, mats):
        import torch
        L = _lib.lib()
        dmats = [m.contiguous() if _is_torch(m) else dev_u32(m) for m in mats]
        n = len(dmats)
        ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in dmats])
        hs = (C.c_size_t * n)(*[m.shape[0] for m in dmats])
        ws = (C.c_size_t * n)(*[m.shape[1] for m in dmats])
        root = np.zeros(8, dtype=np.uint32)
        handle = C.c_void_p()
        torch.cuda.current_stream()
        _lib.check(L.p3hip_mmcs_commit_hiding_dev(self._kind, ptrs, hs, ws, n, self.rng._h, root.ctypes.data_as(C.c_void_p),
                                                  C.byref(handle), _stream_ptr()))
        return root, MerkleTree(handle, dmats, root)

    def open_batch(self, index, tree):
        n = len(tree.mats)
        tot = sum(m.shape[1] + self.SALT_ELEMS for m in tree.mats)
        rows = np.zeros(tot, dtype=np.uint32)
        path = np.zeros((max(tree.log_max_height, 1), 8), dtype=np.uint32)
        _lib.check(_lib.lib().p3hip_mmcs_open_batch(tree._h, index, rows.ctypes.data_as(C.c_void_p),
                                                    path.ctypes.data_as(C.c_void_p), _stream_ptr()))
        vals, salts, off = [], [], 0
        for m in tree.mats:
            w = m.shape[1]
            vals.append(rows[off:off + w].copy())
            salts.append(rows[off + w:off + w + self.SALT_ELEMS].copy())
            off += w + self.SALT_ELEMS
        assert len(vals) == n
        return vals, (salts, path[: tree.log_max_height].copy())

    # the leaf layout of a hiding tree: every salt a width-4 matrix of its matrix's height, m0, s0, m1, s1 ...
    def _salted_dims(self, dims):
        out = []
        for h, w in dims:
            out += [(h, w), (h, self.SALT_ELEMS)]
        return out

    def _columns(self, widths):
        """positions of the value words and of the salt words inside an interleaved row"""
        vals, salts, off = [], [], 0
        for w in widths:
            vals += range(off, off + w)
            salts += range(off + w, off + w + self.SALT_ELEMS)
            off += w + self.SALT_ELEMS
        return vals, salts

    def verify_batch(self, root, dims, index, opened_values, proof):
        """MerkleTreeHidingMmcs::verify_batch: proof = (salts, siblings) as open_batch returns it."""
        salts, path = proof
        parts = []
        for v, s in zip(opened_values, salts):
            parts += [np.asarray(v, dtype=np.uint32).reshape(-1), np.asarray(s, dtype=np.uint32).reshape(-1)]
        if len(parts) != 2 * len(dims):
            raise ValueError("verify_batch: one opened row and one salt per matrix of dims")
        return self._verify(root, self._salted_dims(dims), index, np.concatenate(parts), path)

    def open_batch_many(self, indices, tree):
        """-> (values [n, sum of the widths], (salts [n, n_mats, SALT_ELEMS], paths [n, log_max_height, 8])), device tensors."""
        import torch
        rows, paths = self._open_many(indices, tree)
        vc, sc = self._columns([m.shape[1] for m in tree.mats])
        vi = torch.tensor(vc, dtype=torch.long, device=rows.device)
        si = torch.tensor(sc, dtype=torch.long, device=rows.device)
        return rows[:, vi].contiguous(), (rows[:, si].reshape(rows.shape[0], len(tree.mats), self.SALT_ELEMS).contiguous(), paths)

    def verify_batch_many(self, root, dims, indices, values, proof, form=0, with_rejected=False):
        """values / proof = (salts, paths) as open_batch_many returns them; dims = the matrices' own (height, width)."""
        import torch
        salts, paths = proof
        vc, sc = self._columns([int(d[1]) for d in dims])
        n = values.shape[0]
        rows = torch.empty((n, len(vc) + len(sc)), dtype=values.dtype, device=values.device)
        rows[:, torch.tensor(vc, dtype=torch.long, device=values.device)] = values.reshape(n, -1)
        rows[:, torch.tensor(sc, dtype=torch.long, device=values.device)] = salts.reshape(n, -1)
        return self._verify_many(root, self._salted_dims(dims), indices, rows, paths, form, with_rejected)
