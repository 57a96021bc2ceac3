"""The code generation p2f::internal_rounds rests on (csrc/poseidon2_f64.hip.h), checked on the gfx950 assembly of mmcs.hip through
tools/isa_histogram.py.  No GPU: hipcc cross-compiles the device side (about 20 s, once for the module).

Every lane update of the internal rounds is meant to be ONE v_fma_f64.  That holds only while the constant table d_c is loaded into
SGPR pairs: were it emitted as a private constant, its entries would become literals and every use a v_fmac_f64 plus a v_mov_b64 copy
of the addend (about 300 copies in compress_layer_f64_kernel), with every result unchanged and every other test green.  The counts
below are the ones profiles/hash_instruction_floor_dyadic.txt states."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import field_ref as F
import poseidon2_dyadic_ref as D

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(F.ROOT, "tools", "isa_histogram.py"),
                          os.path.join(F.ROOT, "plonky3-mobile_amd", "csrc", "mmcs.hip"), "compress_layer_f64", "leaf_hash_f64_kernel",
                          "poseidon2_permute_f64", "compress_layer_q4"], check=True, capture_output=True, text=True).stdout
    k = json.loads(out)["kernels"]
    pick = lambda needle: next(v for n, v in k.items() if needle in n)  # noqa: E731
    return {n: pick(n) for n in ("compress_layer_f64_kernel", "leaf_hash_f64_kernel", "poseidon2_permute_f64_kernel", "compress_layer_q4_kernel")}


def _count(kernel, prefix):
    return sum(v for m, v in kernel["by_mnemonic"].items() if m.startswith(prefix))


def test_compress_kernel_has_no_register_copies_and_fits_eight_waves(kernels):
    k = kernels["compress_layer_f64_kernel"]
    assert _count(k, "v_mov_b64") == 0, k["by_mnemonic"]
    assert k["private_segment_fixed_size"] == 0 and not _count(k, "scratch_")
    assert k["vgpr_count"] <= 64  # eight waves per SIMD: __launch_bounds__(256, 8)
    assert kernels["poseidon2_permute_f64_kernel"]["vgpr_count"] <= 64 and kernels["leaf_hash_f64_kernel"]["vgpr_count"] <= 64


def test_compress_kernel_executes_the_schedules_operation_count(kernels):
    """13 + 25 v_fract_f64 (one per lane sum, one per dyadic fold) and 13 + 16 v_rndne_f64 (one per reduce) in the unrolled rounds, none
    elsewhere in the kernel; and the dynamic VALU count of a wave from the block structure: entry + 4 x the first external loop + the
    unrolled internal rounds + 4 x the second loop + the stores = the 3997 the counters read."""
    k = kernels["compress_layer_f64_kernel"]
    n_dy = sum(len(v) for v in D.DYADIC_FOLDS.values())
    n_int = sum(len(v) for v in D.INTEGER_FOLDS.values())
    assert _count(k, "v_fract_f64") == 13 + n_dy == 38 and _count(k, "v_rndne_f64") == 13 + n_int == 29
    loops = [b for b in k["blocks"] if b["loops_back_to"] == b["label"]]
    assert len(loops) == 2, k["blocks"]  # the two external-round loops stay rolled, the internal rounds are straight-line code
    ext = 16 * 19 + 64  # sixteen S-boxes and one external linear layer per trip
    internal = 13 * 19 + D.OPS_PER_PERMUTATION
    assert loops[0]["valu"] == ext + internal, (loops[0]["valu"], internal)  # the loop body and what it falls through to
    assert k["static_valu"] + 3 * ext + 3 * ext == 3997


def test_quad_form_keeps_its_code(kernels):
    """the quad form reads the same table: it holds a handful of copies, not the 130 it gets when d_c's entries become literals"""
    assert _count(kernels["compress_layer_q4_kernel"], "v_mov_b64") <= 8
