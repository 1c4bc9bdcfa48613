// token_exp.hpp -- EXP, the f32 exponential of the token readout (include/dllm_quant.h 8h), shared
// by the kernels of token.hip and the host mirror in host_rules.cpp (and usable without HIP: the
// exhaustive check tests/cpp/token_host_check.cpp includes it from a plain C++ program).
//
// Domain: d <= 0, -inf and NaN.  Built only from f32 add, multiply and fmaf (each rounded once;
// compile with -ffp-contract=off), one exact scaling by 2^k and integer ops, so any IEEE binary32
// host reproduces the bits.
//   EXP(NaN) = the quiet NaN 0x7fc00000.
//   EXP(d)   = +0 for every d < kExpCut = -87 (-inf included).  exp(-87) = 1.39 * 2^-126, so every
//              result above the cut-off is a normal number: no denormal is ever produced.
//   Otherwise, argument reduction (Cody-Waite, two steps):
//     t  = RN(d * 0x1.715476p+0f)                              (log2 e)
//     kf = RN(RN(t + 0x1.8p+23f) - 0x1.8p+23f)                 (t to the nearest integer, ties to even;
//                                                               -126 <= kf <= 0)
//     r  = fmaf(kf, -0x1.62e400p-1f, d)                        (ln 2's high part, 16 bits: kf * hi exact)
//     r  = fmaf(kf, -0x1.7f7d1cp-20f, r)                       (ln 2's low part); |r| <= 0.3467
//   the degree-7 Taylor polynomial, Horner form, one fmaf per step:
//     p = 1/5040; p = fmaf(p, r, 1/720); p = fmaf(p, r, 1/120); p = fmaf(p, r, 1/24);
//     p = fmaf(p, r, 1/6); p = fmaf(p, r, 1/2); p = fmaf(p, r, 1); p = fmaf(p, r, 1)
//   with the coefficients 0x1.a01a02p-13f, 0x1.6c16c2p-10f, 0x1.111112p-7f, 0x1.555556p-5f,
//   0x1.555556p-3f, 0.5f, 1.0f, 1.0f (truncation error <= 0.3467^8 / 40320 = 5.2e-9), and
//     EXP(d) = RN(p * 2^kf), 2^kf built from its bits ((kf + 127) << 23): exact, since p * 2^kf is normal.
//   EXP(0) = EXP(-0) = 1 exactly (t = kf = r = 0, p = 1).
// Largest error against the exact exponential, measured over every f32 in [-87, 0] (1 118 699 521
// values, tests/cpp/token_host_check.cpp --exhaustive): 0.937081 ulp of the result, at
// d = -0x1.79082cp+2 (kExpUlps below is that figure rounded up).
#pragma once

#include <cstdint>

#include "rule_hd.hpp"

namespace dllm {
namespace token {

constexpr float kExpCut = -87.0f;
// The measured largest error of EXP in units in the last place of the result (the exhaustive sweep
// prints it; tests/test_token_readout_cpu.py asserts the sweep stays at or below this figure).
constexpr float kExpUlps = 0.9371f;

// The body for d in [-87, 0] (callers handle NaN and the cut-off).  On the device RN-to-integer and
// the scaling are single instructions (v_rndne_f32, v_ldexp_f32) with the values of the two-add form
// and of the multiply by 2^kf: both exact operations, the same bits.
DLLM_HD float exp_body(float d) {
    const float t = d * 0x1.715476p+0f;
#if defined(__HIP_DEVICE_COMPILE__)
    const float kf = __builtin_rintf(t);
#else
    const float kf = (t + 0x1.8p+23f) - 0x1.8p+23f;
#endif
    float r = __builtin_fmaf(kf, -0x1.62e400p-1f, d);
    r = __builtin_fmaf(kf, -0x1.7f7d1cp-20f, r);
    float p = 0x1.a01a02p-13f;
    p = __builtin_fmaf(p, r, 0x1.6c16c2p-10f);
    p = __builtin_fmaf(p, r, 0x1.111112p-7f);
    p = __builtin_fmaf(p, r, 0x1.555556p-5f);
    p = __builtin_fmaf(p, r, 0x1.555556p-3f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_ldexpf(p, static_cast<int>(kf));
#else
    const uint32_t scale = static_cast<uint32_t>(static_cast<int32_t>(kf) + 127) << 23;
    return p * __builtin_bit_cast(float, scale);
#endif
}

DLLM_HD float exp_le0(float d) {
    if (d != d) return __builtin_bit_cast(float, 0x7fc00000u);
    if (d < kExpCut) return 0.0f;
    return exp_body(d);
}

#if defined(__HIPCC__)
// exp_le0 for a d known not to be NaN, without a branch: the body runs on max(d, -87) (device only:
// it is the form the kernels' hot loops use; the same bits as exp_le0 for every non-NaN d <= 0).
__device__ inline __attribute__((always_inline)) float exp_le0_nonan(float d) {
    const float e = exp_body(d < kExpCut ? kExpCut : d);
    return d < kExpCut ? 0.0f : e;
}
#endif

}  // namespace token
}  // namespace dllm
