"""CPU tests of the host verifier of caller-defined AIRs (include/p3hip.h p3hip_air_proof_len, p3hip_air_verify; csrc/air_verifier_dev.hip)
against the reference prover and verifier of tests/air_ref.py and the package's own verify_air, and of the C and C++ mirrors.
Nothing here touches a GPU: both entries are host code."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import air_many as AM
import air_ref as A
import pcs_many as M
import test_gpu_air as TG
from conftest import ROOT

P = AM.P
# every FRI tuple tests/test_gpu_air.py uses, once
TUPLES = sorted(set(TG.FRI_SETS) | {t for _, _, t in TG.CASES_BC} | {(1, 0, 4, 2), (1, 1, 4, 2), (2, 0, 3, 1), (3, 0, 3, 1)})


@pytest.fixture(scope="module")
def airs(p3, oracle):
    return A.all_airs(p3)


@pytest.mark.parametrize("name", AM.NAMES)
def test_proof_len_is_the_reference_provers_and_its_proofs_are_accepted(p3, airs, name):
    air = airs[name][0]
    seen = 0
    for hash, kind in AM.HASHES:
        for log_n in (1, 2, 3):
            for t in TUPLES:
                if not AM.applies(air, log_n, t):
                    continue
                proof, pis = AM.ref_proof(airs, name, kind, log_n, t)
                fp = p3.FriParameters(*t)
                what = (name, hash, log_n, t)
                assert p3.air_proof_len(air, log_n, fp, hash) == len(proof), what
                assert air.verify(proof, pis, log_n, fp, hash) == 0 == A.verify(kind, t, air.code, air.consts, air.width, proof, pis, log_n), what
                seen += 1
    assert seen >= 12


def test_every_gate_of_proof_len_is_refused_by_name(p3, airs):
    fib, d = airs["fib"][0], airs["D"][0]
    fp = p3.FriParameters

    def refused(air, log_n, t, hash, msg):
        with pytest.raises(p3.P3HipError, match=msg) as e:
            p3.air_proof_len(air, log_n, fp(*t), hash)
        assert e.value.code == -1

    refused(fib, 0, (1, 0, 4, 2), "poseidon2", r"air_proof_len: log_n must lie in 1\.\.27 for this AIR")
    refused(fib, 28, (1, 0, 4, 2), "poseidon2", r"air_proof_len: log_n must lie in 1\.\.27 for this AIR")
    refused(d, 25, (3, 0, 4, 2), "keccak", r"air_proof_len: log_n must lie in 1\.\.24 for this AIR \(the quotient domain has 2\^\(log_n \+ 3\) points\)")
    refused(d, 3, (2, 0, 4, 2), "poseidon2", "air_proof_len: log_blowup 2 is below the AIR's log_quotient_degree 3")
    refused(fib, 3, (0, 0, 4, 2), "poseidon2", r"pcs verify: LDE height outside \[2\^2, 2\^27\]")
    refused(fib, 27, (1, 0, 4, 2), "poseidon2", r"pcs verify: LDE height outside \[2\^2, 2\^27\]")
    refused(fib, 3, (1, 3, 4, 2), "poseidon2", "pcs verify: log_final_poly_len must be below the matrices' log height")
    refused(fib, 3, (1, 0, 4, 31), "poseidon2", "pcs verify: proof_of_work_bits too large")
    refused(fib, 3, (1, 0, 0, 0), "poseidon2", "pcs verify: num_queries must be positive")
    with pytest.raises(p3.P3HipError, match="pcs verify: unknown hash configuration"):
        p3._lib.check(p3._lib.lib().p3hip_air_proof_len(fib._h, 2, 3, fp(1, 0, 4, 2)._c(), C.byref(C.c_size_t())))
    with pytest.raises(p3.P3HipError, match="air_proof_len: null argument"):
        p3._lib.check(p3._lib.lib().p3hip_air_proof_len(fib._h, 0, 3, fp(1, 0, 4, 2)._c(), None))
    # a trace too wide for one open: 2 x 4096 + 4 batched columns
    b = p3.AirBuilder(4096, 0)
    b.assert_zero(b.local(0))
    refused(b.build(), 3, (1, 0, 4, 2), "poseidon2", "round 1 matrix 0 point 0: more than 8192 batched columns")


def _verify_air_code(p3, air, proof, pis, log_n, fp, hash):
    try:
        p3.verify_air(air, proof, pis, log_n, fp, hash)
    except p3.AirRejected as e:
        return e.code
    return 0


CASES = [("fib", 3, (1, 0, 4, 2)), ("B", 2, (2, 1, 4, 2)), ("C", 3, (2, 0, 4, 3)), ("D", 3, (3, 0, 3, 1))]


@pytest.mark.parametrize("name,log_n,t", CASES)
@pytest.mark.parametrize("hash,kind", AM.HASHES)
def test_verify_answers_as_verify_air_on_every_kind_of_changed_word(p3, airs, name, log_n, t, hash, kind):
    air = airs[name][0]
    proof, pis = AM.ref_proof(airs, name, kind, log_n, t)
    fp = p3.FriParameters(*t)
    w, C = air.width, air.n_chunks
    head = A.header_words(w, air.log_quotient_degree)
    hk = AM.header_kinds(w, C)
    classes = AM.word_classes(kind, t, log_n, w, C)
    assert len(classes) * 4 == len(proof)
    rng = np.random.default_rng(len(name) + kind)
    pick = lambda offs: int(offs[int(rng.integers(len(offs)))])
    cases = [("magic", AM.with_word(proof, 0)), ("version", AM.with_word(proof, 1)), ("log_n", AM.with_word(proof, 2))]
    cases += [("count %d" % o, AM.with_word(proof, o)) for o in hk["count"]]
    cases += [(k, AM.with_word(proof, pick(hk[k]))) for k in ("root", "local", "next", "chunk")]
    cases += [(k + " = P", AM.with_word(proof, pick(hk[k]), P)) for k in ("root", "local", "next", "chunk")]
    cases += [("truncated to %d bytes" % n, proof[:n]) for n in (0, 3, 4, 8, 12, 4 * 7, 4 * 19, 4 * 20 + 2, 4 * (21 + 4 * w), 4 * (head - 17), 4 * head - 4, 4 * head - 1)]
    cases += [("header only", proof[:4 * head])]
    fri = classes[head:]
    for cls in (M.SHAPE, M.FELT, M.DIGEST):
        offs = np.nonzero(fri == cls)[0]
        if len(offs):  # under Poseidon2 the digests are field words: no DIGEST class
            cases.append(("FRI class %d" % cls, AM.with_word(proof, head + pick(offs))))
    codes = set()
    for what, bad in cases:
        got = air.verify(bad, pis, log_n, fp, hash)
        assert got == _verify_air_code(p3, air, bad, pis, log_n, fp, hash) != 0, (what, got)
        if len(bad) == len(proof):  # the reference reader pads a truncated proof its own way
            ref = A.verify(kind, t, air.code, air.consts, air.width, bad, pis, log_n)
            assert ref != 0 and (got == ref or min(got, ref) < 10), (what, got, ref)  # the header codes are verify_air's own
        codes.add(got)
    assert {1, 2, 3, 4, 10} <= codes, codes
    assert p3.take_last_error() is None  # Air.verify takes its rejection's message


@pytest.mark.parametrize("name,log_n,t", CASES)
def test_wrong_public_values_are_an_ood_mismatch_and_one_above_p_is_refused(p3, airs, name, log_n, t):
    air = airs[name][0]
    fp = p3.FriParameters(*t)
    for hash, kind in AM.HASHES:
        proof, pis = AM.ref_proof(airs, name, kind, log_n, t)
        for i in range(air.n_public):
            wrong = pis.copy()
            wrong[i] = (int(wrong[i]) + 1) % P
            assert air.verify(proof, wrong, log_n, fp, hash) == 10 == A.verify(kind, t, air.code, air.consts, air.width, proof, wrong, log_n)
            assert _verify_air_code(p3, air, proof, wrong, log_n, fp, hash) == 10
            for v in (P, 0xFFFFFFFF):
                wrong[i] = v
                with pytest.raises(p3.P3HipError, match="air_verify: public value %d is not a canonical field element" % i) as e:
                    air.verify(proof, wrong, log_n, fp, hash)
                assert e.value.code == -1
        for bad_log_n in (0, 28 - air.log_quotient_degree):
            with pytest.raises(p3.P3HipError, match="air_verify: log_n must lie in") as e:
                air.verify(proof, pis, bad_log_n, fp, hash)
            assert e.value.code == -1


def test_header_with_the_new_declarations_is_plain_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "air_verify.c"
    src.write_text('''#include "p3hip.h"
int use(const p3hip_air_t *air, const p3hip_fri_params_t *fp, const uint8_t *proof, size_t len, const uint32_t *pis, uint32_t *st) {
    size_t n = 0;
    int code = 0;
    p3hip_air_verifier_t *v = 0;
    const uint8_t *ptrs[1];
    ptrs[0] = proof;
    if (p3hip_air_proof_len(air, P3HIP_HASH_KECCAK, 3, fp, &n) || p3hip_air_verify(air, P3HIP_HASH_KECCAK, 3, fp, proof, len, pis, &code)) return -1;
    if (p3hip_air_verifier_create(air, P3HIP_HASH_KECCAK, 3, fp, 4, &v)) return -2;
    code += p3hip_air_verifier_verify(v, 1, ptrs, &len, pis, st);
    code += p3hip_air_verifier_verify_dev(v, proof, n, 0, pis, 1, st, 0, 0);
    code += p3hip_air_eval_ext_dev((p3hip_air_t *)0, 0, pis, pis, pis, pis, pis, 0, st);
    p3hip_air_verifier_destroy(v);
    return code == P3HIP_VERIFY_MALFORMED;
}
int main(void) { return 0; }
''')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cpp_mirror_verifies_on_the_host(p3, airs, tmp_path):
    """p3hip::air_proof_len and p3hip::air_verify run (host code); p3hip::AirVerifier compiles: its methods are named, never called."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    t, log_n = (1, 0, 4, 2), 3
    proof, pis = AM.ref_proof(airs, "fib", 0, log_n, t)
    air = airs["fib"][0]
    arr = lambda words: ", ".join("%du" % int(v) for v in words)
    src = tmp_path / "air_verify.cpp"
    src.write_text('''#include <cstdio>
#include "p3hip.hpp"
static std::vector<uint32_t> many(p3hip::AirVerifier& v, const std::vector<std::vector<uint8_t>>& proofs, const std::vector<uint32_t>& pis) {
    v.verify_many_dev(nullptr, v.proof_len(), nullptr, nullptr, 0, nullptr, nullptr, nullptr);
    return v.verify_many(proofs, pis);
}
int main(int argc, char**) {
    using namespace p3hip;
    const std::vector<uint32_t> code = {%s}, pis = {%s}, words = {%s};
    Air air(2, 3, code, std::vector<uint32_t>{});
    FriParameters fp{%d, %d, %d, %d};
    std::vector<uint8_t> proof((const uint8_t*)words.data(), (const uint8_t*)words.data() + 4 * words.size());
    std::printf("len %%zu\\n", air_proof_len(air, %d, fp));
    std::printf("accept %%d\\n", air_verify(air, proof, pis, %d, fp));
    proof[0] ^= 1;
    std::printf("magic %%d\\n", air_verify(air, proof, pis, %d, fp));
    try { air_proof_len(air, 0, fp); } catch (const Error& e) { std::printf("refused %%s\\n", e.what()); }
    if (argc > 100) { AirVerifier v(air, %d, fp); many(v, {proof}, pis); }
    return 0;
}
''' % ((arr(air.code.reshape(-1)), arr(pis), arr(np.frombuffer(proof, np.uint32))) + t + (log_n,) * 4))
    exe = tmp_path / "air_verify"
    libdir = os.path.dirname(p3._lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lp3hip", "-Wl,-rpath," + libdir,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[:3] == ["len %d" % len(proof), "accept 0", "magic 1"], r.stdout
    assert lines[3].startswith("refused ") and "air_proof_len: log_n must lie in 1..27" in lines[3], r.stdout
