// C++ host program over include/p3hip.hpp: proves a CALLER's FibonacciAir trace with caller public values, as the reference
// calls prove(&config, &FibonacciAir {}, trace, &pis) (native/src/fib_air.rs:61,68-70).  The trace is built here on the host.
//   - a Fibonacci trace with its own public values gives the bytes of prove(a, b), and verify accepts them;
//   - with the check, a corrupted trace is refused with the row that breaks a rule;
//   - without it, the corrupted trace is proven (as upstream release builds do) and verify rejects the proof.
// Build: g++ -std=c++17 -O2 -Iinclude tools/prove_trace_demo.cpp -Lplonky3-mobile_amd -lp3hip -Wl,-rpath,... -o tools/_bin/prove_trace_demo
#include <cstdio>
#include <cstdlib>

#include "p3hip.hpp"

using namespace p3hip;

static RowMajorMatrix fib_trace(uint64_t a, uint64_t b, size_t n) {  // fib_air.rs:266-284 generate_trace_rows
    std::vector<uint32_t> v(2 * n);
    uint64_t l = a % P, r = b % P;
    for (size_t i = 0; i < n; i++) {
        v[2 * i] = to_monty(l);
        v[2 * i + 1] = to_monty(r);
        const uint64_t t = (l + r) % P;
        l = r;
        r = t;
    }
    return RowMajorMatrix(std::move(v), 2);
}

int main(int argc, char** argv) {
    try {
        auto avail = is_available();
        std::printf("%s\n", avail.second.c_str());
        if (!avail.first) return 2;
        const unsigned log_n = argc > 1 ? (unsigned)std::atoi(argv[1]) : 10;
        const size_t n = (size_t)1 << log_n;
        const FriParameters fp{1, 0, 20, 8};
        FibAirProver prover(log_n, fp);
        const uint64_t a = 3, b = 4, x = fib_public_x(a, b, n);
        const uint64_t pis[3] = {a, b, x};
        RowMajorMatrix trace = fib_trace(a, b, n);
        const std::vector<uint8_t> proof = prover.prove_trace(trace, pis, true);
        if (proof != prover.prove(a, b)) { std::printf("FAIL prove_trace bytes differ from prove(a, b)\n"); return 3; }
        verify_fib_air(proof, a, b, x, log_n, fp);
        std::printf("prove_trace ok (n=%zu, x=%llu, %zu bytes)\n", n, (unsigned long long)x, proof.size());

        const size_t row = n / 2;
        trace.values[2 * row + 1] = to_monty(12345);
        try {
            prover.prove_trace(trace, pis, true);
            std::printf("FAIL the checked prover took a corrupted trace\n");
            return 4;
        } catch (const Error& e) {
            std::printf("expected error: %s\n", e.what());
            if (std::string(e.what()).find("row " + std::to_string(row - 1)) == std::string::npos) { std::printf("FAIL row\n"); return 5; }
        }
        const std::vector<uint8_t> bad = prover.prove_trace(trace, pis);
        try {
            verify_fib_air(bad, a, b, x, log_n, fp);
            std::printf("FAIL verify accepted the proof of a corrupted trace\n");
            return 6;
        } catch (const Error& e) {
            std::printf("expected rejection: %s\n", e.what());
        }
        std::printf("OK\n");
        return 0;
    } catch (const Error& e) {
        std::printf("FAIL %s\n", e.what());
        return 1;
    }
}
