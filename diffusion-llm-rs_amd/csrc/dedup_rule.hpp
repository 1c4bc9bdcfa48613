// dedup_rule.hpp -- the constants of the dedup rules (include/dllm_quant.h 8i) shared by the kernels
// of dedup.hip and the host mirror in capi_host.cpp (plain C++: usable without HIP).
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

#if defined(__HIPCC__)
#define DLLM_DEDUP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DLLM_DEDUP_HD inline
#endif

namespace dllm {
namespace dedup {

constexpr uint64_t kEmptyKey = ~uint64_t(0);
constexpr uint64_t kNoSeq = ~uint64_t(0);
constexpr size_t kHeaderWords = 4;
constexpr size_t kFlagWord = 0, kCountWord = 1, kSideWord = 2;
constexpr size_t kMaxDim = 65535;

constexpr bool is_pow2(size_t n) { return n != 0 && (n & (n - 1)) == 0; }
constexpr size_t table_words(size_t slots) { return kHeaderWords + 2 * slots; }

// The slot a probe starts at.  The hash's low bits are a short sum of the last few codes (31^k b),
// so they are mixed with the high ones first: a multiply by 2^64 / phi, the high word folded down.
DLLM_DEDUP_HD size_t first_slot(uint64_t h, size_t mask) {
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

}  // namespace dedup
}  // namespace dllm
