// rule_hd.hpp -- DLLM_HD marks a function of a rule header: one body for the kernels and for the plain
// C++ mirror in host_rules.cpp (a host and device function under hipcc, an inline function otherwise).
#pragma once

#if defined(__HIPCC__)
#define DLLM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DLLM_HD inline
#endif
