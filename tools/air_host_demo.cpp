// p3hip::Air (include/p3hip.hpp) over the C ABI, host code only: creation, info(), eval_ext and a refusal.  No GPU is touched.
//   g++ -std=c++17 -Iinclude tools/air_host_demo.cpp -Lplonky3-mobile_amd -lp3hip
// Prints the AIR's figures, the four words of eval_ext on fixed operands, and the message of a refused program; tests/test_air_cpp_host.py
// compares them with the Python binding and the reference evaluator.
#include <cstdio>

#include "p3hip.hpp"

int main() {
    using namespace p3hip;
    const auto op = air_operand;
    // width 2, one public, one constant: is_first_row * (local[0] - public[0]) = 0;  is_transition * (local[0] * local[1] + k - next[0]) = 0
    const std::vector<uint32_t> code = {
        P3HIP_AIR_OP_SUB, 0, op(P3HIP_AIR_KIND_LOCAL, 0), op(P3HIP_AIR_KIND_PUBLIC, 0),
        P3HIP_AIR_OP_MUL, 0, op(P3HIP_AIR_KIND_SELECTOR, P3HIP_AIR_SEL_FIRST_ROW), op(P3HIP_AIR_KIND_SLOT, 0),
        P3HIP_AIR_OP_ASSERT_ZERO, 0, op(P3HIP_AIR_KIND_SLOT, 0), 0,
        P3HIP_AIR_OP_MUL, 0, op(P3HIP_AIR_KIND_LOCAL, 0), op(P3HIP_AIR_KIND_LOCAL, 1),
        P3HIP_AIR_OP_ADD, 1, op(P3HIP_AIR_KIND_SLOT, 0), op(P3HIP_AIR_KIND_CONST, 0),
        P3HIP_AIR_OP_SUB, 0, op(P3HIP_AIR_KIND_SLOT, 1), op(P3HIP_AIR_KIND_NEXT, 0),
        P3HIP_AIR_OP_MUL, 1, op(P3HIP_AIR_KIND_SELECTOR, P3HIP_AIR_SEL_TRANSITION), op(P3HIP_AIR_KIND_SLOT, 0),
        P3HIP_AIR_OP_ASSERT_ZERO, 0, op(P3HIP_AIR_KIND_SLOT, 1), 0,
    };
    try {
        Air air(2, 1, code, {to_monty(7)});
        const p3hip_air_info_t& i = air.info();
        printf("info %u %u %u %u %u %u %u chunks %zu\n", i.width, i.n_public, i.n_instructions, i.n_constraints, i.n_slots, i.max_degree,
               i.log_quotient_degree, air.n_chunks());
        std::vector<uint32_t> local(8), next(8);
        std::array<uint32_t, 12> sels{};
        std::array<uint32_t, 4> alpha{};
        for (uint32_t k = 0; k < 8; k++) { local[k] = to_monty(3 + 5 * k); next[k] = to_monty(1000 + 11 * k); }
        for (uint32_t k = 0; k < 12; k++) sels[k] = to_monty(77 + 13 * k);
        for (uint32_t k = 0; k < 4; k++) alpha[k] = to_monty(900001 + k);
        const auto out = air.eval_ext(local, next, {to_monty(123456)}, sels, alpha);
        printf("eval %u %u %u %u\n", out[0], out[1], out[2], out[3]);
        try {
            air.eval_ext(local, {1, 2, 3}, {to_monty(1)}, sels, alpha);
            return 1;
        } catch (const Error& e) {
            printf("expected error: %s\n", e.what());
        }
    } catch (const Error& e) {
        printf("FAILED: %s\n", e.what());
        return 1;
    }
    try {
        std::vector<uint32_t> bad = code;
        bad[4 * 3 + 3] = op(P3HIP_AIR_KIND_LOCAL, 2);  // a column past the width
        Air air(2, 1, bad, {to_monty(7)});
        return 1;
    } catch (const Error& e) {
        printf("refused %d: %s\n", e.code, e.what());
    }
    printf("OK\n");
    return 0;
}
