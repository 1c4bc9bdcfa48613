// search_rule.hpp -- what the cosine search (include/dllm_quant.h 8g) states once for the kernels of
// search.hip and the host mirror in host_rules.cpp (plain C++: usable without HIP): the limits of the
// store, the key order and the argument checks the device and the _host entry points share.  The
// neighbour and dedup rules take the store's limits from here.
#pragma once

#include <cstddef>
#include <cstdint>

#include "dllm_quant.h"
#include "error.hpp"
#include "rule_hd.hpp"

namespace dllm {
namespace search {

constexpr size_t kMaxK = 256;
constexpr size_t kMaxDim = 65535;
constexpr size_t kMaxRows = size_t(1) << 31;   // a row's index is an int32

// A float's bits, in the form of HIP's __float_as_uint (a copy taken by value): the select kernel
// compiles to the same instructions as with that intrinsic, which a bit_cast of s in place does not.
DLLM_HD uint32_t float_bits(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, sizeof(b));
    return b;
}

// (score descending, index ascending) as one u64 ascending: the score's bits made orderable in the
// high word (-0 folded into +0, every NaN below -inf), the complemented index in the low word.
// Index < 2^31 keeps the low word >= 2^31, so the key 0 is free to mean "no row".
DLLM_HD uint64_t search_key(float s, uint32_t idx) {
    uint32_t b = float_bits(s);
    uint32_t ord;
    if (s != s) {
        ord = 0u;
    } else {
        if (b == 0x80000000u) b = 0u;
        ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return (static_cast<uint64_t>(ord) << 32) | static_cast<uint32_t>(~idx);
}

// ---- argument checks: the device entry point and its _host twin call the same function (static: a
// translation unit's own copy, so the library exports none of them) ----

static inline int check_store_shape(size_t rows, size_t dim) {
    if (dim == 0 || dim > kMaxDim) return fail(DLLM_ERR_INVALID_PARAMS, "dim must be between 1 and 65535");
    if (rows >= kMaxRows) return fail(DLLM_ERR_SHAPE_MISMATCH, "rows must be below 2^31 (the index is an int32)");
    return DLLM_OK;
}

static inline int check_k(size_t k) {
    if (k == 0 || k > kMaxK) return fail(DLLM_ERR_INVALID_PARAMS, "k must be between 1 and 256");
    return DLLM_OK;
}

}  // namespace search
}  // namespace dllm
