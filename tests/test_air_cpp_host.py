"""The C++ mirror p3hip::Air (include/p3hip.hpp) over the C ABI: tools/air_host_demo.cpp compiled with g++ and run as a child process.
Everything it calls is host code, so it runs without a GPU; its figures are compared with the Python binding and the reference
evaluator of tests/air_ref.py on the same program and operands."""
import os
import subprocess

import numpy as np

import air_ref as A
from conftest import ROOT

BIN = os.path.join(ROOT, "tools", "_bin", "air_host_demo")


def test_cpp_air_mirror_creates_evaluates_and_refuses(p3, oracle):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    libdir = os.path.dirname(p3._lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "air_host_demo.cpp"),
                           "-L" + libdir, "-lp3hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines()}
    # the same AIR through the Python builder: the figures agree, and the value with both evaluators
    b = p3.AirBuilder(2, 1)
    b.when_first_row().assert_eq(b.local(0), b.public(0))
    b.when_transition().assert_zero(b.local(0) * b.local(1) + b.const(7) - b.next(0))
    air = b.build()
    assert lines["info"].split()[1:] == [str(v) for v in (2, 1, 8, 2, 2, 3, 1)] + ["chunks", "2"]
    assert (air.n_constraints, air.max_degree, air.log_quotient_degree) == (2, 3, 1)
    m = lambda vals: oracle.to_monty(np.array(vals, dtype=np.uint64))
    local, nxt = m([3 + 5 * k for k in range(8)]), m([1000 + 11 * k for k in range(8)])
    sels, alpha, pis = m([77 + 13 * k for k in range(12)]), m([900001 + k for k in range(4)]), m([123456])
    want = air.eval_ext(local, nxt, pis, sels, alpha)
    assert np.array_equal(want, A.eval_ext(air.code, air.consts, local, nxt, pis, sels, alpha))
    assert [int(v) for v in lines["eval"].split()[1:]] == [int(v) for v in want]
    assert "width x 4 words per row" in lines["expected"]
    assert lines["refused"].startswith("refused -1: air_create: instruction 3: operand b: column 2 out of range (width 2)")
