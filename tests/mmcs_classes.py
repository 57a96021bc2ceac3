"""The driver logic of mmcs_commit — which rows are hashed into which digest — as an independent driver, a grid of commitments and the
names the grid must reach.  No GPU here.

  driver_layers   an independent per-digest tree driver over the oracle's primitives only (hash_row / compress or their Keccak
                  forms): tests/pyref.py::merkle_layers with the hash as a parameter.  It keeps oracle.Tree, the reference of the
                  GPU tests, honest on the shapes of the grid (tests/test_mmcs_classes_host.py).
  the grid        the commitments tests/test_gpu_mmcs_classes.py runs, shared with the host test: one injected matrix at every
                  level (A), two and all injections (B), class compositions on both sides of the cooperative threshold (C), 64
                  matrices (D), hiding commitments, and the caps.
  kernels_of ..   every kernel mmcs_commit can launch, by hash and profile: what the host test asks the grid to reach.  Which of
                  them a shape DOES reach is the library's own answer (plan.mmcs_commit_plan), never restated here.

A shape is a list of (height, width) in the CALLER's order; a class is the matrices of one height in that order."""
import zlib

import numpy as np

P = 0x78000001
HASHES = ("poseidon2", "keccak")
PROFILES = ("latency", "throughput")
SALT_ELEMS = 4


# ---------------------------------------------------------------- the independent driver
def driver_layers(oracle, mats, kind):
    """Digest layers of MerkleTreeMmcs::commit(mats), leaf layer first, as numpy (len, 8) arrays.  kind: "poseidon2" | "keccak".
    Leaf i = hash(row i of every tallest matrix, concatenated in caller order); next[i] = compress(prev[2i], prev[2i+1]), and where
    some matrix has that layer's length, compress(that, hash(rows i of that class)).  An empty row hashes like any other."""
    hash_row, compress = {"poseidon2": (oracle.hash_row, oracle.compress), "keccak": (oracle.keccak_hash_row, oracle.keccak_compress)}[kind]
    mats = [np.asarray(m, dtype=np.uint32) for m in mats]
    maxh = max(m.shape[0] for m in mats)

    def rows_hash(h, i):
        return hash_row(np.concatenate([m[i] for m in mats if m.shape[0] == h]))

    layers = [np.stack([rows_hash(maxh, i) for i in range(maxh)])]
    while len(layers[-1]) > 1:
        prev, n = layers[-1], len(layers[-1]) // 2
        inject = any(m.shape[0] == n for m in mats)
        nxt = []
        for i in range(n):
            d = compress(prev[2 * i], prev[2 * i + 1])
            if inject:
                d = compress(d, rows_hash(n, i))
            nxt.append(d)
        layers.append(np.stack(nxt))
    return layers


def matrices(case_id, dims):
    """Seeded random words below P, one matrix per entry of dims.  The seed is the case and the matrix's place in it, never the
    order of calls: structured data would let a kernel that reads the wrong row or the wrong matrix pass."""
    out = []
    for k, (h, w) in enumerate(dims):
        rng = np.random.default_rng([zlib.crc32(case_id.encode()), k, h, w])
        out.append(rng.integers(0, P, size=(h, w), dtype=np.uint64).astype(np.uint32))
    return out


def salted_dims(dims):
    """the leaf layout of a hiding commitment: m0, s0, m1, s1 ... every salt a width-4 matrix of its matrix's height"""
    out = []
    for h, w in dims:
        out += [(h, w), (h, SALT_ELEMS)]
    return out


# ---------------------------------------------------------------- the grid
GRID_A_LOG_HEIGHTS = list(range(1, 15)) + [16]


def grid_a(log_h):
    """one injected matrix at every level below 2^log_h.  2^14 is the smallest top height with a layer on each side of 2^10, 2^11 and
    2^12; 2^16 adds layers above the quad form's range."""
    return [("A-%d-%d" % (log_h, j), [(1 << log_h, 3), (1 << j, 5)]) for j in range(log_h)]


# Where the issue's grid ends, two names of the coverage accounting are still out of reach; these shapes reach them.  A compression
# layer is past the quad form (latency profile) only from 2^16 digests OUT, so from a 2^17-row tree: compress_layer_f64.
GRID_A_EXTRA = [("A-17-9", [(1 << 17, 3), (1 << 9, 5)])]

B_TOP = 13
B_INTERLEAVED = [5, 13, 0, 9, 2, 11, 7, 4, 12, 1, 8, 3, 10, 6]


def grid_b_pairs():
    """two injections below 2^13, every pair of levels"""
    return [("B-%d-%d" % (j1, j2), [(1 << B_TOP, 2), (1 << j1, 3), (1 << j2, 1)]) for j1 in range(B_TOP) for j2 in range(j1 + 1, B_TOP)]


def grid_b_all():
    """a matrix at every level, in descending, ascending and interleaved caller order (the order inside a commitment is the caller's)"""
    m = lambda k: (1 << k, 1 + k % 3)
    return [("B-all-descending", [m(k) for k in range(B_TOP, -1, -1)]), ("B-all-ascending", [m(k) for k in range(B_TOP + 1)]),
            ("B-all-interleaved", [m(k) for k in B_INTERLEAVED])]


C_CLASS_LOG_HEIGHTS = (5, 12)  # the two sides of the cooperative threshold 2^12: leaf_hash against leaf_hash_f64_rowset
C_WIDTHS = [
    [1] * 16,                                       # the cap
    [8, 3], [7, 1], [9, 8, 7],                      # boundaries on, before and after the Poseidon2 rate of 8
    [34, 1], [33, 1], [35, 34], [17, 17, 1],        # the Keccak rate block of 34 words; an odd total: the last u64's high half is empty
    [70, 35, 1], [64, 64], [68, 2],                 # wide matrices that are not alone: the wide leaf kernels must not be taken
    [70], [68], [64],                               # ... and alone: they must (the accounting asks for both wide leaf kernels)
    [4, 4], [6, 4], [8, 4], [4] * 8,                # the salted shapes, in a plain commitment
    [5, 4], [4, 5], [8, 4, 4], [4] * 7, [4, 4, 4, 4, 4, 4, 6, 4], [4] * 4,  # their near-misses
    [3, 0, 2], [0],                                 # a zero-width matrix inside a class, and alone
]


def _wname(ws):
    return "x".join(str(w) for w in ws)


def grid_c(log_h):
    """every composition once as the leaf class and once as an injected class under a (2 h, 2) matrix"""
    h = 1 << log_h
    out = []
    for ws in C_WIDTHS:
        out.append(("C-%d-leaf-%s" % (log_h, _wname(ws)), [(h, w) for w in ws]))
        out.append(("C-%d-injected-%s" % (log_h, _wname(ws)), [(2 * h, 2)] + [(h, w) for w in ws]))
    return out


def grid_d():
    """64 matrices, seven classes of at most ten: as listed, reversed, and scaled to a tallest height of 2^13"""
    base = [(1 << (k // 10), 1 + k % 5) for k in range(64)]
    return [("D-listed", base), ("D-reversed", base[::-1]), ("D-scaled", [(h << 7, w) for h, w in base])]


HIDING_LOG_HEIGHTS = (5, 12)


def grid_hiding(log_h):
    """hiding commitments (the matrices' own dims; the tree is over salted_dims): classes of 1, 2, 4, 8 matrices of one width.  Eight
    fill the class cap with sixteen entries; width 4 times four is the salted<4,4> shape, the single matrices of 4, 6, 8 words the
    salted<W,1> shapes, the rest falls to the generic kernels."""
    return [("H-%d-%dx%d" % (log_h, k, w), [(1 << log_h, w)] * k) for k in (1, 2, 4, 8) for w in (4, 5, 6, 8)]


HIDING_MIXED = [("H-mixed", [(1 << 12, 6), (1 << 12, 6), (1 << 7, 4), (1 << 3, 8)])]


def plain_grid():
    """every plain commitment of the grid"""
    out = []
    for lh in GRID_A_LOG_HEIGHTS:
        out += grid_a(lh)
    out += GRID_A_EXTRA + grid_b_pairs() + grid_b_all()
    for lh in C_CLASS_LOG_HEIGHTS:
        out += grid_c(lh)
    return out + grid_d()


def hiding_grid():
    out = []
    for lh in HIDING_LOG_HEIGHTS:
        out += grid_hiding(lh)
    return out + HIDING_MIXED


def tallest(dims):
    return max(h for h, _ in dims)


# ---------------------------------------------------------------- which kernels a shape reaches
MAX_CLASS_MATS, MAX_MATS = 16, 64

POSEIDON2_KERNELS = {"leaf_coop", "leaf_hash_q4", "leaf_hash_f64_wide", "leaf_hash_f64", "leaf_hash_f64_rowset", "leaf_hash",
                     "tree_levels_coop", "compress_layer_q4", "compress_layer_f64", "compress_layer"}
KECCAK_KERNELS = {"keccak_leaf_wide", "keccak_leaf_salted<4,1>", "keccak_leaf_salted<6,1>", "keccak_leaf_salted<8,1>",
                  "keccak_leaf_salted<4,4>", "keccak_leaf", "keccak_tree_levels_coop", "keccak_tree_levels", "keccak_compress"}
LATENCY_ONLY = {"leaf_hash_q4", "compress_layer_q4"}
THROUGHPUT_ONLY = {"keccak_tree_levels"}
MULTI_LEVEL = {"tree_levels_coop": 5, "keccak_tree_levels_coop": 4, "keccak_tree_levels": 2}  # name -> the most levels of one launch


def kernels_of(kind, profile):
    """every kernel mmcs_commit can launch for a hash under a profile"""
    names = POSEIDON2_KERNELS if kind == "poseidon2" else KECCAK_KERNELS
    return names - (THROUGHPUT_ONLY if profile == "latency" else LATENCY_ONLY)


def launch_neighbours(dims, launches):
    """per launch above the leaves (plan.mmcs_commit_plan's list): (kernel, levels, its input layer is an injected one, the layer after its last one is an injected one).
    The leaf layer is no injected layer."""
    maxh = tallest(dims)
    lens = [maxh >> i for i in range(maxh.bit_length())]
    heights = {h for h, _ in dims}
    out, l = [], 1
    for name, levels in launches:
        after = l - 1 >= 1 and lens[l - 1] in heights
        before = l + levels < len(lens) and lens[l + levels] in heights
        out.append((name, levels, after, before))
        l += levels
    assert l == len(lens), "the launches of a plan cover every layer once"
    return out
