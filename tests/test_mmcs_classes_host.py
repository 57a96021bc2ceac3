"""The grid of tests/test_gpu_mmcs_classes.py, checked without a GPU: (1) oracle.Tree, the reference of the GPU tests, against an
independent per-digest driver on every member small enough for one; (2) the grid as a condition — over the library's own launch
plan (p3hip_mmcs_commit_plan: what mmcs_commit executes), it reaches every kernel the commit can launch, every `levels` value, and
each multi-level kernel on both sides of an injected layer, under both profiles.  If a name is missing here, the grid is wrong.
(3) The plan itself, on shapes worked out by hand from csrc/mmcs.hip, alignment and stride branches included."""
import numpy as np
import pytest

import mmcs_classes as mc

HOST_MAX_HEIGHT = 1 << 8


def _kind(oracle, hash_name):
    return oracle.HASH_KECCAK if hash_name == "keccak" else oracle.HASH_POSEIDON2


def test_the_grid_is_the_one_the_issue_lists():
    """counts and caps, so that an edit of the grid that drops shapes is seen"""
    assert sum(len(mc.grid_a(lh)) for lh in mc.GRID_A_LOG_HEIGHTS) == 121
    assert len(mc.grid_b_pairs()) == 78 and len(mc.grid_b_all()) == 3
    assert sorted(mc.B_INTERLEAVED) == list(range(mc.B_TOP + 1))
    for _, dims in mc.grid_b_all():
        assert sorted(dims) == sorted((1 << k, 1 + k % 3) for k in range(14))
    assert len(mc.grid_c(5)) == 2 * len(mc.C_WIDTHS) and len(mc.C_WIDTHS) == 26
    for case_id, dims in mc.grid_d():
        assert len(dims) == mc.MAX_MATS, case_id
        assert max(sum(1 for h, _ in dims if h == hh) for hh, _ in dims) == 10 and len({h for h, _ in dims}) == 7, case_id
    assert [mc.tallest(d) for _, d in mc.grid_d()] == [1 << 6, 1 << 6, 1 << 13]
    every = mc.plain_grid()
    assert len({case_id for case_id, _ in every}) == len(every)  # the ids seed the matrices
    assert any(sum(1 for h, _ in dims if h == mc.tallest(dims)) == mc.MAX_CLASS_MATS for _, dims in every)        # the class cap, as leaves
    assert any(sum(1 for h, _ in dims if h == mc.tallest(dims) // 2) == mc.MAX_CLASS_MATS for _, dims in every)   # and injected
    hid = mc.hiding_grid()
    assert len(hid) == 33
    assert any(len(mc.salted_dims(dims)) == mc.MAX_CLASS_MATS for _, dims in hid)


@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_oracle_trees_equal_the_independent_driver(oracle, hash_name):
    """every grid member of at most 2^8 rows (all 36 (H, j) pairs with H <= 8, the 16-matrix class, the 64-matrix commitments, the
    salted shapes and their near-misses, a zero-width matrix alone, inside a class and as an injected class, the hiding layouts):
    oracle.mmcs_commit's root and EVERY layer equal driver_layers, digest for digest"""
    cases = [(c, d) for c, d in mc.plain_grid() if mc.tallest(d) <= HOST_MAX_HEIGHT]
    cases += [(c + "-salted", mc.salted_dims(d)) for c, d in mc.hiding_grid() if mc.tallest(d) <= HOST_MAX_HEIGHT]
    assert len(cases) >= 86
    assert {c for c, _ in cases} >= {"A-8-0", "A-8-7", "C-5-leaf-" + "x".join(["1"] * 16), "C-5-leaf-0", "C-5-leaf-3x0x2", "C-5-injected-0", "D-reversed"}
    for case_id, dims in cases:
        mats = mc.matrices(case_id, dims)
        root, tree = oracle.mmcs_commit(mats, _kind(oracle, hash_name))
        want = mc.driver_layers(oracle, mats, hash_name)
        got = tree.layers()
        assert len(got) == len(want) == mc.tallest(dims).bit_length(), case_id
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (hash_name, case_id, len(w))
        assert np.array_equal(root, want[-1][0]), (hash_name, case_id)


def test_an_empty_row_hashes_to_the_zero_digest(oracle):
    """what upstream's sponges return for no input, and what a zero-width class therefore injects"""
    empty = np.zeros(0, dtype=np.uint32)
    assert not oracle.hash_row(empty).any() and not oracle.keccak_hash_row(empty).any()


@pytest.mark.parametrize("profile", mc.PROFILES)
@pytest.mark.parametrize("hash_name", mc.HASHES)
def test_the_grid_reaches_every_kernel_and_every_levels_value(p3, hash_name, profile):
    """coverage accounting over the library's plan: a condition on the grid, not a measurement"""
    shapes = list(mc.plain_grid())
    shapes += [(c, mc.salted_dims(d)) for c, d in mc.hiding_grid()]
    reached, levels_seen, before, after = set(), {}, set(), set()
    for case_id, dims in shapes:
        leaf, launches = p3.plan.mmcs_commit_plan(hash_name, profile, dims)
        reached.add(leaf)
        for name, levels, is_after, is_before in mc.launch_neighbours(dims, launches):
            reached.add(name)
            assert levels >= 1, (case_id, name)
            if name in mc.MULTI_LEVEL:
                assert levels <= mc.MULTI_LEVEL[name], (case_id, name, levels)
                levels_seen.setdefault(name, set()).add(levels)
                if is_before:
                    before.add(name)
                if is_after:
                    after.add(name)
            else:
                assert levels == 1, (case_id, name, levels)
    want = mc.kernels_of(hash_name, profile)
    assert reached == want, (sorted(want - reached), sorted(reached - want))
    multi = {n: top for n, top in mc.MULTI_LEVEL.items() if n in want}
    assert set(multi) == set(levels_seen)
    for name, top in multi.items():
        assert levels_seen[name] == set(range(1, top + 1)), (name, sorted(levels_seen[name]))
    assert before == set(multi) and after == set(multi), (sorted(before), sorted(after))


def test_the_kernel_lists_are_the_issues():
    """every name, spelled out once more: the accounting above compares against exactly these, by hash and profile"""
    assert mc.kernels_of("poseidon2", "latency") == {"leaf_coop", "leaf_hash_q4", "leaf_hash_f64_wide", "leaf_hash_f64", "leaf_hash_f64_rowset",
                                                     "leaf_hash", "tree_levels_coop", "compress_layer_q4", "compress_layer_f64", "compress_layer"}
    assert mc.kernels_of("poseidon2", "throughput") == {"leaf_coop", "leaf_hash_f64_wide", "leaf_hash_f64", "leaf_hash_f64_rowset", "leaf_hash",
                                                        "tree_levels_coop", "compress_layer_f64", "compress_layer"}
    salted = {"keccak_leaf_salted<4,1>", "keccak_leaf_salted<6,1>", "keccak_leaf_salted<8,1>", "keccak_leaf_salted<4,4>"}
    assert mc.kernels_of("keccak", "latency") == salted | {"keccak_leaf_wide", "keccak_leaf", "keccak_tree_levels_coop", "keccak_compress"}
    assert mc.kernels_of("keccak", "throughput") == salted | {"keccak_leaf_wide", "keccak_leaf", "keccak_tree_levels_coop", "keccak_tree_levels",
                                                              "keccak_compress"}
    assert mc.MULTI_LEVEL == {"tree_levels_coop": 5, "keccak_tree_levels_coop": 4, "keccak_tree_levels": 2}


def test_plan_on_shapes_read_off_the_source(p3):
    """a few plans worked out by hand from mmcs_commit, so that the plan is not only compared with itself"""
    plan = p3.plan.mmcs_commit_plan
    # Poseidon2, 2^14 rows, injection at 2^10: quad leaves and quad layers 2^13, 2^12 (latency); 2^11 alone before the injected layer;
    # then 2^9 .. 2^5 in one launch and 2^4 .. 2^0 in the next
    dims = [(1 << 14, 3), (1 << 10, 5)]
    assert plan("poseidon2", "latency", dims) == ("leaf_hash_q4", [("compress_layer_q4", 1), ("compress_layer_q4", 1), ("tree_levels_coop", 1),
                                                                      ("compress_layer", 1), ("tree_levels_coop", 5), ("tree_levels_coop", 5)])
    assert plan("poseidon2", "throughput", dims) == ("leaf_hash_f64", [("compress_layer_f64", 1), ("compress_layer_f64", 1), ("tree_levels_coop", 1),
                                                                          ("compress_layer", 1), ("tree_levels_coop", 5), ("tree_levels_coop", 5)])
    # Keccak, the same shape: per-lane compressions down to 2^12; throughput: 2^12 -> 2^11 by the per-lane levels kernel (one level: the
    # injected 2^10 follows), then cooperative levels of at most four; latency: cooperative from 2^12 digests in
    assert plan("keccak", "throughput", dims) == ("keccak_leaf", [("keccak_compress", 1), ("keccak_compress", 1), ("keccak_tree_levels", 1),
                                                                     ("keccak_compress", 1), ("keccak_tree_levels_coop", 4),
                                                                     ("keccak_tree_levels_coop", 4), ("keccak_tree_levels_coop", 2)])
    assert plan("keccak", "latency", dims) == ("keccak_leaf", [("keccak_compress", 1), ("keccak_compress", 1), ("keccak_tree_levels_coop", 1),
                                                                  ("keccak_compress", 1), ("keccak_tree_levels_coop", 4),
                                                                  ("keccak_tree_levels_coop", 4), ("keccak_tree_levels_coop", 2)])
    # no injection below 2^13 under Keccak / throughput: 2^12 -> 2^10 in one per-lane launch of two levels
    assert plan("keccak", "throughput", [(1 << 13, 70)]) == ("keccak_leaf_wide", [("keccak_compress", 1), ("keccak_tree_levels", 2),
                                                                                     ("keccak_tree_levels_coop", 4), ("keccak_tree_levels_coop", 4),
                                                                                     ("keccak_tree_levels_coop", 2)])
    # two rows: one launch of one level whatever the hash
    assert plan("poseidon2", "latency", [(2, 3), (1, 5)]) == ("leaf_coop", [("compress_layer", 1)])
    assert plan("keccak", "latency", [(2, 3)]) == ("keccak_leaf", [("keccak_tree_levels_coop", 1)])
    # a hiding class of four 4-word matrices is the salted<4,4> shape; of four 6-word ones it is not
    assert plan("keccak", "latency", mc.salted_dims([(32, 4)] * 4))[0] == "keccak_leaf_salted<4,4>"
    assert plan("keccak", "latency", mc.salted_dims([(32, 6)] * 4))[0] == "keccak_leaf"
    assert plan("keccak", "latency", mc.salted_dims([(32, 6)]))[0] == "keccak_leaf_salted<6,1>"


A = 0x7F0000001000  # a made-up 4096-byte-aligned address: the plan looks at alignment only and dereferences nothing
PAIR = [(32, 6), (32, 4)]      # one (matrix, salt) pair
PAIR4 = [(32, 4), (32, 4)]
BOTH = ("latency", "throughput")
# (hash, profiles, dims, strides, matrix addresses, layers address, leaf kernel): the branches on an address's alignment or a row
# stride, read off mmcs_plan / salted_width in csrc/mmcs.hip
ALIGNMENT_AND_STRIDE_CASES = [
    ("poseidon2", ("latency",), [(1 << 13, 3)], None, None, A, "leaf_hash_q4"),            # layers 16-byte aligned
    ("poseidon2", ("latency",), [(1 << 13, 3)], None, None, A + 8, "leaf_hash_f64"),       # layers at 8 mod 16: no quad leaves
    ("poseidon2", BOTH, [(1 << 13, 64)], None, None, A + 8, "leaf_hash_f64_wide"),
    ("poseidon2", BOTH, [(1 << 5, 3)], None, None, A, "leaf_coop"),
    ("poseidon2", BOTH, [(1 << 5, 3)], [5], None, A, "leaf_hash_f64_rowset"),              # a column group of a wider matrix
    ("poseidon2", BOTH, [(1 << 13, 3)], [5], None, A, "leaf_hash_f64_rowset"),
    ("keccak", BOTH, [(32, 70)], [70], None, A, "keccak_leaf_wide"),
    ("keccak", BOTH, [(32, 70)], [72], None, A, "keccak_leaf"),
    ("keccak", BOTH, PAIR, None, [A + 8, A + 16], A, "keccak_leaf_salted<6,1>"),           # matrix at 0 mod 8, salt at 0 mod 16
    ("keccak", BOTH, PAIR, None, [A + 4, A + 16], A, "keccak_leaf"),                       # matrix at 4 mod 8
    ("keccak", BOTH, PAIR, None, [A + 8, A + 24], A, "keccak_leaf"),                       # salt at 8 mod 16
    ("keccak", BOTH, PAIR, [7, 4], [A, A + 16], A, "keccak_leaf"),                         # an odd matrix stride
    ("keccak", BOTH, PAIR4, None, [A + 8, A + 16], A, "keccak_leaf"),                      # 4-word matrix at 8 mod 16
    ("keccak", BOTH, PAIR4, [6, 4], [A, A + 16], A, "keccak_leaf"),                        # stride 6: rows leave 16-byte alignment
    ("keccak", BOTH, PAIR4 * 4, [4, 4, 4, 4, 4, 8, 4, 4], None, A, "keccak_leaf"),         # one salt's stride is not 4
    ("keccak", BOTH, PAIR4 * 4, None, None, A, "keccak_leaf_salted<4,4>"),                 # ... and the shape it misses
]


@pytest.mark.parametrize("case", ALIGNMENT_AND_STRIDE_CASES, ids=lambda c: "%s-%s-%s" % (c[0], "x".join("%dx%d" % d for d in c[2][:2]), c[6]))
def test_plan_on_alignment_and_stride(p3, case):
    hash_name, profiles, dims, strides, mats, layers, leaf = case
    for profile in profiles:
        assert p3.plan.mmcs_commit_plan(hash_name, profile, dims, strides=strides, mats=mats, layers=layers)[0] == leaf, profile


def test_plan_refuses_what_the_commit_refuses(p3):
    """mmcs_check_shape's own error, and no plan"""
    with pytest.raises(p3.P3HipError, match="more than 16 matrices of one height"):
        p3.plan.mmcs_commit_plan("poseidon2", "latency", [(32, 1)] * 17)
    with pytest.raises(p3.P3HipError, match="row stride below the width"):
        p3.plan.mmcs_commit_plan("keccak", "latency", [(32, 4)], strides=[3])
