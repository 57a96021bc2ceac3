"""CPU tests of the caller-trace entries (include/p3hip.h "a CALLER's trace"): the header declares them with their arities, the
package binds them, and the C++ demo of include/p3hip.hpp's prove_trace builds with g++ and, without a GPU, reports
"HIP unavailable" (no fallback).  The GPU side: tests/test_gpu_prove_trace.py."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "tools", "_bin", "prove_trace_demo")


def _header():
    text = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _arities(code):
    out = {}
    for m in re.finditer(r"\b(p3hip_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return out


def test_header_declares_the_trace_entries():
    text, code = _header()
    fns = _arities(code)
    assert fns["p3hip_fib_check_trace_dev"] == 5
    assert fns["p3hip_fib_prover_prove_trace_dev"] == 6
    assert fns["p3hip_fib_prover_prove_trace"] == 7
    assert fns["p3hip_fib_prover_enqueue_trace_dev"] == 3
    assert fns["p3hip_fib_batch_prove_traces_dev"] == 7
    assert re.search(r"#define\s+P3HIP_PROVE_CHECK_TRACE\s+1u", code)
    assert re.search(r"typedef struct\s*\{\s*int64_t first_bad_row;\s*uint32_t mask;\s*uint64_t bad_rows;\s*\}\s*p3hip_trace_check_t;", code)
    for bit, v in (("FIRST_LEFT", 1), ("FIRST_RIGHT", 2), ("NEXT_LEFT", 4), ("NEXT_RIGHT", 8), ("LAST_RIGHT", 16), ("RANGE", 32)):
        assert re.search(r"#define\s+P3HIP_TRACE_BAD_%s\s+%du" % (bit, v), code), bit
    assert "BUFFER CONTRACT" in text  # the _dev entries' buffer contract is written down


def test_package_binds_the_trace_entries(p3):
    names = set(p3._lib.declared_symbols())
    for n in ("p3hip_fib_check_trace_dev", "p3hip_fib_prover_prove_trace_dev", "p3hip_fib_prover_prove_trace",
              "p3hip_fib_prover_enqueue_trace_dev", "p3hip_fib_batch_prove_traces_dev"):
        assert n in names
    p3._lib.lib()  # every declared symbol resolves in the built library
    assert p3.PROVE_CHECK_TRACE == 1
    assert callable(p3.check_fib_trace)
    assert callable(p3.FibAirProver.prove_trace) and callable(p3.FibAirProver.enqueue_trace)
    assert callable(p3.FibAirBatchProver.prove_traces)


def test_python_argument_checks_need_no_gpu(p3):
    from plonky3_mobile_amd import fib_air
    import ctypes as C
    w = fib_air._monty_pis([1, 0x78000001 + 2, -1])
    assert list(w) == [((1 << 32) % 0x78000001), ((2 << 32) % 0x78000001), (((0x78000000) << 32) % 0x78000001)]
    with pytest.raises(ValueError):
        fib_air._monty_pis([1, 2])
    assert isinstance(w, C.Array)
    with pytest.raises(TypeError):
        fib_air._device_trace([[0, 1]])


def test_rust_front_end_proves_a_caller_trace():
    src = open(os.path.join(ROOT, "integration", "native", "src", "hip_front_end.rs")).read()
    assert "pub fn prove_fib_air_hip(" in src and "p3hip_fib_prover_prove_trace(" in src


def _build(p3):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    libdir = os.path.dirname(p3._lib.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "prove_trace_demo.cpp"), "-L" + libdir, "-lp3hip", "-Wl,-rpath," + libdir,
           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN]
    subprocess.check_call(cmd)


def test_prove_trace_demo_builds_and_refuses_without_gpu(p3):
    _build(p3)
    ok, _ = p3.is_available()
    if ok:
        pytest.skip("GPU present: covered by test_prove_trace_demo_on_gpu")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "HIP unavailable" in r.stdout


@pytest.mark.gpu
def test_prove_trace_demo_on_gpu(p3):
    _build(p3)
    r = subprocess.run([BIN, "12"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "prove_trace ok" in r.stdout and "expected rejection" in r.stdout
