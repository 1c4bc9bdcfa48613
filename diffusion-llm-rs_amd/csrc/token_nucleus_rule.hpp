// token_nucleus_rule.hpp -- the integer part of the top-p / min-p rule (include/dllm_quant.h 8k),
// shared by the threshold search of token.hip and the host mirror in host_rules.cpp: the fixed-point
// weight of an element, the fixed-point forms of the two parameters and the 96-bit comparison.
//   W     = (u64) trunc(g * 2^32) for g = EXP(RN(y - m)) in [0, 1]: the product is exact (a power of two
//           scales it), so W is an integer function of g's bits; W(1) = 2^32, W(+0) = 0.  EXP never
//           exceeds 1 on d <= 0 (tests/cpp/token_exp_monotone.cpp walks every f32 there: no value above
//           1, though 2878 one-ulp steps down), so the conversion below needs 32 bits for every g but 1.
//   pfix  = (u64) floor((double) top_p * 2^32), mfix = (u64) ceil((double) min_p * 2^32): exact in f64.
//   A 2^32 >= pfix T, the nucleus test, in integers of up to 95 bits (A, T < 2^63, pfix <= 2^32).
#pragma once

#include <cstdint>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // __umul64hi, for the device form of the comparison
#endif

#include "token_exp.hpp"

namespace dllm {
namespace token {

// 8k.2: the weight of an element from its g = EXP(RN(y - m)), 0 <= g <= 1.
DLLM_HD uint64_t nucleus_weight(float g) {
    return g < 1.0f ? static_cast<uint64_t>(static_cast<uint32_t>(g * 0x1p32f)) : (uint64_t(1) << 32);
}

// 8k.3: does the mass A (of the elements >= a candidate threshold) reach the share pfix / 2^32 of T?
// A 2^32 >= pfix T as 96-bit integers: the high words, then the low ones.
DLLM_HD bool nucleus_reaches(uint64_t A, uint64_t pfix, uint64_t T) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t hi = __umul64hi(pfix, T), lo = pfix * T;
    const uint64_t ahi = A >> 32, alo = A << 32;
    return ahi > hi || (ahi == hi && alo >= lo);
#else
    return (static_cast<unsigned __int128>(A) << 32) >= static_cast<unsigned __int128>(pfix) * T;
#endif
}

// The smallest A that reaches: ceil(pfix T / 2^32), and at least 1 (pfix == 0, a top_p below 2^-32,
// is reached by the maximum alone, whose weight is 2^32 >= 1; an element of weight 0 never decides).
// A >= nucleus_need(pfix, T) is nucleus_reaches(A, pfix, T) for every A >= 1; the threshold search
// computes it once per row and compares 64-bit sums against it.
DLLM_HD uint64_t nucleus_need(uint64_t pfix, uint64_t T) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t hi = __umul64hi(pfix, T), lo = pfix * T;
#else
    const unsigned __int128 p = static_cast<unsigned __int128>(pfix) * T;
    const uint64_t hi = static_cast<uint64_t>(p >> 64), lo = static_cast<uint64_t>(p);
#endif
    const uint64_t need = (hi << 32) + (lo >> 32) + ((lo & 0xffffffffu) ? 1u : 0u);   // hi < 2^31
    return need ? need : 1u;
}

// The parameters in fixed point (host functions: one f64 product each, exact, then floor / ceil).
inline uint64_t nucleus_pfix(float top_p) {   // 0 < top_p <= 1
    return static_cast<uint64_t>(static_cast<double>(top_p) * 0x1p32);
}
inline uint64_t nucleus_mfix(float min_p) {   // 0 <= min_p <= 1
    const double v = static_cast<double>(min_p) * 0x1p32;
    const uint64_t f = static_cast<uint64_t>(v);
    return f + (static_cast<double>(f) < v ? 1u : 0u);
}

}  // namespace token
}  // namespace dllm
