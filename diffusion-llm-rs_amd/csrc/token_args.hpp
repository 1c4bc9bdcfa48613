// token_args.hpp -- what the token readout and sampling (include/dllm_quant.h 8h, 8j, 8k) state once
// for token.hip and the host mirror in host_rules.cpp (plain C++: usable without HIP): the chunk of
// the summation order and the argument checks the device and the _host entry points share.
#pragma once

#include <cmath>
#include <cstddef>

#include "dllm_quant.h"
#include "error.hpp"

namespace dllm {

constexpr size_t kTokChunk = 16384;   // elements of a chunk: 8f's tree runs over each chunk's 256 lane sums

namespace token {

// V, ld and dtype of the logits; `sampling` picks the wording for an empty vocabulary.
static inline int check_logits(size_t V, size_t ld, int dtype, bool sampling) {
    if (V == 0)
        return fail(DLLM_ERR_INVALID_PARAMS, sampling ? "V == 0: no token to sample from an empty vocabulary"
                                                      : "V == 0: no token to read out of an empty vocabulary");
    if (ld < V) return fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least V");
    if (V >= (size_t(1) << 31)) return fail(DLLM_ERR_SHAPE_MISMATCH, "V must be below 2^31 (the token is an int32)");
    if (dtype != DLLM_F32 && dtype != DLLM_F16) return fail(DLLM_ERR_UNSUPPORTED, "dtype must be DLLM_F32 or DLLM_F16");
    return DLLM_OK;
}

// dllm_token_sample's values; r = 1 / temperature (8j.1: one IEEE division).
static inline int check_sample_args(size_t V, size_t ld, int dtype, float temperature, float &r) {
    if (int rc = check_logits(V, ld, dtype, true)) return rc;
    r = 1.0f / temperature;
    if (!(temperature > 0.0f) || !std::isfinite(temperature) || !std::isfinite(r))
        return fail(DLLM_ERR_INVALID_PARAMS, "temperature and 1 / temperature must be positive and finite");
    return DLLM_OK;
}

// dllm_token_sample_ex's: the same, then the two masks of 8k.
static inline int check_sample_ex_args(size_t V, size_t ld, int dtype, float temperature, float top_p, float min_p,
                                       float &r) {
    if (int rc = check_sample_args(V, ld, dtype, temperature, r)) return rc;
    if (!(top_p > 0.0f) || top_p > 1.0f) return fail(DLLM_ERR_INVALID_PARAMS, "top_p must be in (0, 1]");
    if (!(min_p >= 0.0f) || min_p > 1.0f) return fail(DLLM_ERR_INVALID_PARAMS, "min_p must be in [0, 1]");
    return DLLM_OK;
}

}  // namespace token
}  // namespace dllm
