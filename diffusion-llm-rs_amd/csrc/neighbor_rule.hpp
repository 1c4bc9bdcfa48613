// neighbor_rule.hpp -- the arithmetic of the row-against-row cosine (include/dllm_quant.h 8l) shared
// by the kernels of neighbors.hip and the host mirror in host_rules.cpp (plain C++: usable without HIP).
//
// The pair table is one Entry per row in caller-owned memory (opaque to callers, 8-byte aligned):
// a = s w and b = z w in f64 (w = 1 / |row|, or 0 for a row without a direction) and C1 = sum c.
// Every f64 operation below is one separately rounded IEEE multiply or add: the translation units
// that include this file are built with -ffp-contract=off, and nothing here may be written as an fma.
#pragma once

#include <math.h>

#include <cstddef>
#include <cstdint>

#include "search_rule.hpp"   // the store's limits (k, dim, rows) and their checks

namespace dllm {
namespace neighbor {

struct Entry {
    double a, b;
    uint32_t c1, pad;
};
static_assert(sizeof(Entry) == 24, "the pair table is 24 bytes per row");

DLLM_HD bool finite_f64(double x) { return x - x == 0.0; }   // false for NaN and +-inf

// C1 = sum c and C2 = sum c^2 of the row (exact u32: dim <= 65535), s and z its f32 scale and zero point.
// The f64 sqrt and divide are correctly rounded on the host and on the device (8g relies on the same).
DLLM_HD Entry make_entry(float sf, float zf, uint32_t c1, uint32_t c2, uint32_t dim) {
    const double s = sf, z = zf;
    const double nb2 = ((s * s) * static_cast<double>(c2) + ((2.0 * s) * z) * static_cast<double>(c1)) +
                       (z * z) * static_cast<double>(dim);
    const bool ok = finite_f64(s) && finite_f64(z) && finite_f64(nb2) && nb2 > 0.0;
    Entry e;
    e.c1 = c1;
    e.pad = 0u;
    if (ok) {
        const double w = 1.0 / ::sqrt(nb2);
        e.a = s * w;
        e.b = z * w;
    } else {
        e.a = 0.0;
        e.b = 0.0;
    }
    return e;
}

// D = sum c_r c_t from S' = sum (c_r - 128)(c_t - 128): exact modulo 2^32, and D < 2^32.
DLLM_HD uint32_t dot_from_signed(int32_t sp, uint32_t c1r, uint32_t c1t, uint32_t dim) {
    return static_cast<uint32_t>(sp) + 128u * (c1r + c1t) - 16384u * dim;
}

// score(r, t): symmetric bit for bit (f64 + and x commute; the cross terms meet each other first).
DLLM_HD float score(double ar, double br, uint32_t c1r, double at, double bt, uint32_t c1t, uint32_t D,
                             uint32_t dim) {
    const double cross = (ar * bt) * static_cast<double>(c1r) + (br * at) * static_cast<double>(c1t);
    const double v = ((ar * at) * static_cast<double>(D) + cross) + (br * bt) * static_cast<double>(dim);
    return static_cast<float>(v);
}

// The pair (query j of the block, store row t) is dropped: the query's own row, or below the threshold.
DLLM_HD bool dropped(float s, float threshold, int64_t self_base, size_t j, size_t t) {
    if (self_base >= 0 && static_cast<uint64_t>(self_base) + j == t) return true;
    return !(s >= threshold);
}

// ---- argument checks: the device entry point and its _host twin call the same function (static: a
// translation unit's own copy, so the library exports none of them) ----

static inline int check_table_aligned(const void *table) {
    if (reinterpret_cast<uintptr_t>(table) % 8) return fail(DLLM_ERR_INVALID_PARAMS, "table must be 8-byte aligned");
    return DLLM_OK;
}

// The values of dllm_neighbor_rows, before its "nq == 0: nothing to do".
static inline int check_rows_args(size_t nq, size_t rows, size_t dim, size_t k, float threshold, int64_t self_base) {
    if (int rc = search::check_k(k)) return rc;
    if (int rc = search::check_store_shape(rows, dim)) return rc;
    if (threshold != threshold) return fail(DLLM_ERR_INVALID_PARAMS, "threshold must not be NaN");
    if (self_base < -1) return fail(DLLM_ERR_INVALID_PARAMS, "self_base must be -1 or a row of the store");
    if (self_base >= 0 && (static_cast<uint64_t>(self_base) > rows || nq > rows - static_cast<uint64_t>(self_base)))
        return fail(DLLM_ERR_INVALID_PARAMS, "self_base + nq exceeds rows");
    return DLLM_OK;
}

// Its buffers, after it.
static inline int check_rows_buffers(const uint8_t *qcodes, const void *qtable, const uint8_t *codes, const void *table,
                                     size_t rows, const int32_t *idx, const float *scores) {
    if (!qcodes || !qtable || !idx || !scores || (rows && (!codes || !table)))
        return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(qtable) % 8 || reinterpret_cast<uintptr_t>(table) % 8)
        return fail(DLLM_ERR_INVALID_PARAMS, "qtable and table must be 8-byte aligned");
    return DLLM_OK;
}

}  // namespace neighbor
}  // namespace dllm
