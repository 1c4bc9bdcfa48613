// token_exp_monotone.cpp -- a one-off record, not part of the suite: EXP (csrc/token_exp.hpp) over every
// f32 in [-inf, 0] (2^31 + 1 bit patterns from -inf up to -0, and +0), checking whether it ever decreases
// or exceeds 1.  Were it monotone, min-p's threshold form (include/dllm_quant.h 8k.4) would keep exactly
// the elements with W >= mfix; with no value above 1 the 32-bit conversion of token_nucleus_rule.hpp
// covers every g < 1.  Prints the first counter-examples.  DESIGN.md records the outcome (2878 one-ulp
// decreases, all in (-0.25, 0); no value above 1).
//   c++ -O2 -std=c++17 -ffp-contract=off -Icsrc tests/cpp/token_exp_monotone.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "token_exp.hpp"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

int main() {
    // negative floats ascend as their bit patterns descend: 0xff800000 (-inf) ... 0x80000000 (-0)
    float prev = dllm::token::exp_le0(from_bits(0xff800000u));
    uint64_t n = 1, steps_up = 0;
    int bad = 0, above_one = 0;
    for (uint32_t b = 0xff800000u - 1; b >= 0x80000000u; --b) {
        const float d = from_bits(b), e = dllm::token::exp_le0(d);
        ++n;
        if (!(e >= prev) && bad++ < 8) std::printf("counter-example: EXP(%a) = %a after %a\n", d, e, prev);
        if (e > 1.0f && above_one++ < 8) std::printf("above 1: EXP(%a) = %a\n", d, e);
        steps_up += e > prev;
        prev = e;
    }
    const float z = dllm::token::exp_le0(0.0f);
    ++n;
    if (!(z >= prev) || z != 1.0f) ++bad, std::printf("counter-example at +0: %a after %a\n", z, prev);
    std::printf("%llu values, %llu increases, %d decreases, %d values above 1: EXP is %s on [-inf, 0]\n",
                static_cast<unsigned long long>(n), static_cast<unsigned long long>(steps_up), bad, above_one,
                bad ? "NOT non-decreasing" : "non-decreasing");
    return bad || above_one ? 1 : 0;
}
