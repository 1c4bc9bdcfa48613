// token_sample_rule.hpp -- the integer part of the token sampling rule (include/dllm_quant.h 8j.4),
// shared by the kernels of token.hip and the host mirror in host_rules.cpp: the three uniforms of a
// row.  Philox4x32-10 keyed by (seed lo, seed hi) on the counter (i lo, i hi, 1, 0); the 1 in the
// third word keeps these draws apart from the N(0,1) stream of csrc/diffusion_rng.hpp, whose
// counters are (blk lo, blk hi, 0, 0).  u_l = float(w_l >> 8) * 2^-24: a 24-bit integer and a power
// of two, exact, in [0, 1 - 2^-24]; w_3 is unused.
#pragma once

#include <cstdint>

#include "token_exp.hpp"

namespace dllm {
namespace token {

DLLM_HD void sample_uniforms(uint64_t seed, uint64_t i, float (&u)[3]) {
    uint32_t c0 = static_cast<uint32_t>(i), c1 = static_cast<uint32_t>(i >> 32), c2 = 1u, c3 = 0u;
    uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = static_cast<uint32_t>(p1);
        c2 = n2;
        c3 = static_cast<uint32_t>(p0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    u[0] = static_cast<float>(c0 >> 8) * 0x1p-24f;
    u[1] = static_cast<float>(c1 >> 8) * 0x1p-24f;
    u[2] = static_cast<float>(c2 >> 8) * 0x1p-24f;
}

}  // namespace token
}  // namespace dllm
