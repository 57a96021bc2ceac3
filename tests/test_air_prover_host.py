"""What of AirProver can be checked without a GPU: the six C entries are exported, declared and bound with one arity everywhere; the
Python wrapper refuses bad arguments before it calls the library; the C++ mirror in include/p3hip.hpp compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = {"p3hip_air_prover_create": 8, "p3hip_air_prover_prove_dev": 6, "p3hip_air_prover_prove": 6, "p3hip_air_prover_enqueue_dev": 3,
           "p3hip_air_prover_finish": 3, "p3hip_air_prover_destroy": 1}


def test_the_six_entries_are_exported_declared_and_bound(p3):
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert "typedef struct p3hip_air_prover p3hip_air_prover_t;" in hdr
    for limit in ("2 width + 4 C <= 8192", "log_n + log_blowup <= 26", "log_quotient_degree (the committed LDE", "log_final_poly_len < log_n"):
        assert limit in hdr, limit
    protos = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    arity = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
             for m in re.finditer(r"\b(p3hip_\w+)\s*\(([^;{]*?)\)\s*;", protos, flags=re.S)}
    lib = C.CDLL(p3._lib.LIB_PATH)
    shim = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "integration", "native", "src", "hip_pcs.rs")).read())
    hpp = open(os.path.join(ROOT, "include", "p3hip.hpp")).read()
    for s, n in ENTRIES.items():
        assert arity.get(s) == n, (s, arity.get(s))
        assert hasattr(lib, s), s
        assert len(p3._lib._SIGS[s][1]) == n, s
        m = re.search(r"fn\s+%s\s*\((.*?)\)\s*(?:->\s*[^;]+)?;" % s, shim, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n, s
        assert s + "(" in hpp, s
    assert p3.AirProver is p3.air.AirProver and "AirProver" in p3.__all__


def test_the_wrapper_refuses_bad_arguments_before_any_library_call(p3, monkeypatch):
    air = p3.fibonacci_air()  # host code: no GPU is needed for the program itself

    def no_call():
        raise AssertionError("the library was called")
    monkeypatch.setattr(p3._lib, "lib", no_call)
    for bad in (0, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="log_n must be an integer >= 1"):
            p3.AirProver(air, bad)
    with pytest.raises(TypeError, match="must be a live Air"):
        p3.AirProver("fib", 3)
    with pytest.raises(ValueError, match="unknown hash configuration"):
        p3.AirProver(air, 3, hash="sha256")
    with pytest.raises(ValueError, match="unknown profile"):
        p3.AirProver(air, 3, profile="fast")
    # the arguments of a proof, on an object that stands for a created one
    pr = object.__new__(p3.AirProver)
    pr.log_n, pr.width, pr.n_public, pr._h, pr._own, pr._stream = 3, 2, 3, C.c_void_p(1), True, None
    pis = np.zeros(3, dtype=np.uint32)
    for shape in ((8, 3), (4, 2), (16,), (8, 2, 1)):
        with pytest.raises(ValueError, match=r"a \(8, 2\) trace of 32-bit Montgomery words"):
            pr.prove(np.zeros(shape, dtype=np.uint32), pis)
    with pytest.raises(ValueError, match="expected 3 words, got 2"):
        pr.prove(np.zeros((8, 2), dtype=np.uint32), pis[:2])
    with pytest.raises(ValueError, match="expected 3 words, got 0"):
        pr.prove(np.zeros((8, 2), dtype=np.uint32))
    with pytest.raises(TypeError, match="a torch device tensor"):
        pr.enqueue(np.zeros((8, 2), dtype=np.uint32), pis)
    import torch
    with pytest.raises(ValueError, match="contiguous device tensor"):
        pr.prove(torch.zeros((8, 2), dtype=torch.int32), pis)  # host memory
    with pytest.raises(ValueError, match=r"a \(8, 2\) trace"):
        pr.prove(torch.zeros((8, 2), dtype=torch.float32), pis)
    pr._h = None  # nothing to destroy


def test_the_cpp_mirror_compiles(p3):
    src = """#include "p3hip.hpp"
std::vector<uint8_t> all_of_it(const p3hip::Air& air, const uint32_t* d_trace, const std::vector<uint32_t>& host, const std::vector<uint32_t>& pis) {
    p3hip::AirProver pr(air, 5, p3hip::FriParameters(), P3HIP_HASH_KECCAK, P3HIP_PROFILE_THROUGHPUT, nullptr, true);
    std::vector<uint8_t> a = pr.prove_dev(d_trace, pis, true), b = pr.prove(host, pis);
    pr.enqueue_dev(d_trace, pis);
    std::vector<uint8_t> c = pr.finish();
    a.insert(a.end(), b.begin(), b.end());
    a.insert(a.end(), c.begin(), c.end());
    return a;
}
"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"],
                       input=src, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
