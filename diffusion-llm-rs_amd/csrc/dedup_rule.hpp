// dedup_rule.hpp -- the constants of the dedup rules (include/dllm_quant.h 8i) shared by the kernels
// of dedup.hip and the host mirror in host_rules.cpp (plain C++: usable without HIP).
//
// The seen-set is one array of u64 words in caller-owned memory:
//   word 0        flag: nonzero once a row found no slot (only a dishonest `base` gets there)
//   word 1        the number of distinct hashes the set holds
//   word 2        the value slot of the one reserved key (kEmptyKey itself, which no key slot can hold)
//   word 3        unused
//   4 .. 4+S      keys[S]: kEmptyKey, or a hash
//   4+S .. 4+2S   vals[S]: the smallest sequence number offered with that hash (kNoSeq while empty)
// kEmptyKey is 2^64 - 1 and not 0: the all-zero row, the common duplicate, hashes to 0 and takes an
// ordinary slot; and "empty" and "no sequence number yet" are the same all-ones byte pattern.
#pragma once

#include <cstddef>
#include <cstdint>

#include "search_rule.hpp"   // the store's limits (dim, rows)

namespace dllm {
namespace dedup {

constexpr uint64_t kEmptyKey = ~uint64_t(0);
constexpr uint64_t kNoSeq = ~uint64_t(0);
constexpr size_t kHeaderWords = 4;
constexpr size_t kFlagWord = 0, kCountWord = 1, kSideWord = 2;
using search::kMaxDim;
using search::kMaxRows;
constexpr uint64_t kMaxSeq = uint64_t(1) << 62;   // sequence numbers (base + row) stay below it
constexpr size_t kMaxSlots = size_t(1) << 56;

constexpr bool is_pow2(size_t n) { return n != 0 && (n & (n - 1)) == 0; }
constexpr size_t table_words(size_t slots) { return kHeaderWords + 2 * slots; }

// The slot a probe starts at.  The hash's low bits are a short sum of the last few codes (31^k b),
// so they are mixed with the high ones first: a multiply by 2^64 / phi, the high word folded down.
DLLM_HD size_t first_slot(uint64_t h, size_t mask) {
    uint64_t m = h * 0x9E3779B97F4A7C15ull;
    m ^= m >> 32;
    return static_cast<size_t>(m) & mask;
}

// 31^e mod 2^64 by squaring (host side and compile time; the kernels read tables built from it).
constexpr uint64_t pow31(uint64_t e) {
    uint64_t r = 1, b = 31;
    while (e) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}
// 31 is odd, so it has an inverse mod 2^64 (Newton: x <- x (2 - 31 x) doubles the correct bits).
constexpr uint64_t inv31() {
    uint64_t x = 31;   // 31 * 31 = 961 = 1 mod 8: three bits to start from
    for (int i = 0; i < 6; ++i) x *= 2 - 31 * x;
    return x;
}
static_assert(inv31() * 31 == 1, "inverse of 31 mod 2^64");

// ---- argument checks: the device entry point and its _host twin call the same function (static: a
// translation unit's own copy, so the library exports none of them) ----

constexpr bool slots_ok(size_t slots) { return is_pow2(slots) && slots <= kMaxSlots; }

static inline int check_dim(size_t dim, size_t ld) {
    if (dim == 0 || dim > kMaxDim) return fail(DLLM_ERR_INVALID_PARAMS, "dim must be between 1 and 65535");
    if (ld < dim) return fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least dim");
    return DLLM_OK;
}

static inline int check_hash_args(size_t rows, size_t dim, size_t ld) {
    if (int rc = check_dim(dim, ld)) return rc;
    if (rows >= kMaxRows) return fail(DLLM_ERR_SHAPE_MISMATCH, "rows must be below 2^31");
    return DLLM_OK;
}

static inline int check_slots(size_t slots) {
    if (!slots_ok(slots)) return fail(DLLM_ERR_INVALID_PARAMS, "slots must be a power of two");
    return DLLM_OK;
}

static inline int check_table_aligned(const void *table) {
    if (reinterpret_cast<uintptr_t>(table) % 8) return fail(DLLM_ERR_INVALID_PARAMS, "table must be 8-byte aligned");
    return DLLM_OK;
}

// The values of dllm_dedup_rows, before its "rows == 0: nothing to do"; table == null is the one-shot form.
static inline int check_filter_args(size_t rows, uint64_t base, const void *table, size_t slots) {
    if (rows >= kMaxRows) return fail(DLLM_ERR_SHAPE_MISMATCH, "rows must be below 2^31 (a kept row's index is an int32)");
    if (base >= kMaxSeq) return fail(DLLM_ERR_INVALID_PARAMS, "base must be below 2^62");
    if (table) {
        if (int rc = check_slots(slots)) return rc;
        if (int rc = check_table_aligned(table)) return rc;
        if (base + rows > slots / 2)
            return fail(DLLM_ERR_INVALID_PARAMS, "base + rows exceeds slots / 2: the seen-set is kept at most half full");
    }
    return DLLM_OK;
}

static inline int check_gather_args(size_t dim, size_t ld, size_t out_ld) {
    if (int rc = check_dim(dim, ld)) return rc;
    if (out_ld < dim) return fail(DLLM_ERR_INVALID_PARAMS, "out_ld must be at least dim");
    return DLLM_OK;
}

}  // namespace dedup
}  // namespace dllm
