// token_host_check.cpp -- a stand-alone driver (its own main) of the token readout's host side.
//
//   token_host_check               dllm_token_readout_host (csrc/host_rules.cpp) on exact-size heap
//                                  buffers, meant to be compiled with host_rules.cpp under the address
//                                  and undefined-behaviour sanitizers: a read or write past an end is
//                                  caught; the values are checked for what needs no second
//                                  implementation (the literal fold, Z >= 1, sum p ~ 1, p_token = 1 / Z,
//                                  padding never read, row independence, the rejections), and EXP at
//                                  its special points and on a strided sample.
//   token_host_check --exhaustive  EXP (csrc/token_exp.hpp) against the exact exponential over every
//                                  f32 in [-87, 0]; prints the largest error in ulps of the result.
//                                  The exact value is glibc's f64 exp (within one f64 ulp: 2^-29 of an
//                                  f32 ulp).  Needs only token_exp.hpp: no library.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "token_exp.hpp"

using dllm::token::exp_le0;

static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// Error of EXP(d) in ulps of the f32 result's binade against exp(d) in f64.
static double ulp_error(float d) {
    const double want = std::exp(static_cast<double>(d));
    const float got = exp_le0(d);
    int e;
    std::frexp(want, &e);                        // want = f * 2^e, f in [0.5, 1): ulp = 2^(e - 24)
    return std::fabs(static_cast<double>(got) - want) / std::ldexp(1.0, e - 24);
}

static int exhaustive() {
    const uint32_t lo = 0x80000000u, hi = 0xc2ae0000u;    // -0 ... -87, ascending bit patterns
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : (nt > 16 ? 16 : nt);
    std::vector<double> worst(nt, 0.0);
    std::vector<uint32_t> where(nt, 0);
    std::vector<uint64_t> bad(nt, 0);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            for (uint64_t b = static_cast<uint64_t>(lo) + t; b <= hi; b += nt) {
                const float d = from_bits(static_cast<uint32_t>(b));
                const float got = exp_le0(d);
                if (!(got >= 0x1p-126f && got <= 1.0f)) ++bad[t];          // never denormal, zero, above 1 or NaN
                const double u = ulp_error(d);
                if (u > worst[t]) worst[t] = u, where[t] = static_cast<uint32_t>(b);
            }
        });
    for (auto &th : pool) th.join();
    double w = 0;
    uint32_t at = 0;
    uint64_t nbad = 0;
    for (unsigned t = 0; t < nt; ++t) {
        nbad += bad[t];
        if (worst[t] > w) w = worst[t], at = where[t];
    }
    std::printf("values %llu\n", static_cast<unsigned long long>(static_cast<uint64_t>(hi) - lo + 1));
    std::printf("out_of_range %llu\n", static_cast<unsigned long long>(nbad));
    std::printf("max_ulp_error %.6f at %a (0x%08x)\n", w, from_bits(at), at);
    return nbad ? 1 : 0;
}

#ifndef TOKEN_CHECK_EXP_ONLY
#include "dllm_quant.h"

static int failed = 0, checked = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checked;                                                    \
        if (!(cond)) {                                                \
            ++failed;                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                             \
    } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {   // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}
static float rndf() { return static_cast<float>(rnd() >> 8) / 8388608.0f - 1.0f; }

static uint16_t to_half(float f) {   // values used here are exactly representable: k / 64, |k| <= 1024
    const uint32_t b = bits(f);
    if ((b & 0x7fffffffu) == 0) return static_cast<uint16_t>(b >> 16);
    const int e = static_cast<int>((b >> 23) & 0xff) - 127 + 15;
    return static_cast<uint16_t>(((b >> 16) & 0x8000u) | (static_cast<uint32_t>(e) << 10) | ((b >> 13) & 0x3ffu));
}

static int32_t fold(const float *x, size_t V) {   // the reference's max_by, literally
    size_t cur = 0;
    for (size_t i = 1; i < V; ++i)
        if (!(x[cur] > x[i])) cur = i;
    return static_cast<int32_t>(cur);
}

static void run(size_t M, size_t V, size_t ld, int dtype, int special) {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> x(M * V);
    for (auto &v : x) v = std::floor(rndf() * 512.0f) / 64.0f;      // multiples of 1/64 in [-8, 8): exact in f16
    if (special == 1 && V > 2) x[V / 2] = std::nanf(""), x[0] = 100.0f;
    if (special == 2)
        for (size_t i = 0; i < V; ++i) x[i] = -inf;
    if (special == 3) x[V - 1] = inf;
    // exact-size buffers: the last row has V elements, not ld; padding holds NaN and +inf
    const size_t total = (M - 1) * ld + V;
    std::vector<float> f32(dtype == DLLM_F32 ? total : 0);
    std::vector<uint16_t> f16(dtype == DLLM_F16 ? total : 0);
    for (size_t i = 0; i < total; ++i) {
        const size_t b = i / ld, c = i % ld;
        if (dtype == DLLM_F32)
            f32[i] = c < V ? x[b * V + c] : (c % 2 ? inf : std::nanf(""));
        else
            f16[i] = c < V ? (x[b * V + c] != x[b * V + c] ? 0x7e00 : std::isinf(x[b * V + c]) ? (x[b * V + c] > 0 ? 0x7c00 : 0xfc00) : to_half(x[b * V + c]))
                           : (c % 2 ? 0x7c00 : 0x7e00);
    }
    const void *logits = dtype == DLLM_F32 ? static_cast<const void *>(f32.data()) : static_cast<const void *>(f16.data());
    std::vector<int32_t> tok(M), tok2(M);
    std::vector<float> st(2 * M), st2(2 * M), p(M * V);
    CHECK(dllm_token_readout_host(logits, dtype, M, V, ld, tok.data(), st.data(), p.data()) == DLLM_OK);
    CHECK(dllm_token_readout_host(logits, dtype, M, V, ld, tok2.data(), st2.data(), nullptr) == DLLM_OK);
    CHECK(std::memcmp(tok.data(), tok2.data(), M * sizeof(int32_t)) == 0);
    CHECK(std::memcmp(st.data(), st2.data(), 2 * M * sizeof(float)) == 0);
    for (size_t b = 0; b < M; ++b) {
        const float *row = &x[b * V];
        CHECK(tok[b] == fold(row, V));
        const bool plain = special == 0 || b > 0;
        if (plain) {
            const float m = st[2 * b], Z = st[2 * b + 1];
            CHECK(m == row[tok[b]] && Z >= 1.0f && Z <= static_cast<float>(V));
            double sum = 0;
            for (size_t i = 0; i < V; ++i) sum += p[b * V + i];
            CHECK(std::fabs(sum - 1.0) < 1e-5);
            // x[tok] == m, so EXP(0) == 1 and p_token = RN(1 / Z)
            CHECK(bits(p[b * V + static_cast<size_t>(tok[b])]) == bits(1.0f / Z));
        } else if (special == 1 && V > 2) {
            CHECK(bits(st[0]) == 0x7fc00000u && bits(st[1]) == 0x7fc00000u && bits(p[0]) == 0x7fc00000u);
        } else if (special == 2) {
            CHECK(st[0] == -inf && bits(st[1]) == 0u && bits(p[V - 1]) == 0x7fc00000u && tok[0] == static_cast<int32_t>(V - 1));
        } else if (special == 3) {
            CHECK(st[0] == inf && bits(st[1]) == 0x7fc00000u && tok[0] == static_cast<int32_t>(V - 1));
        }
    }
    if (M > 1) {   // a row on its own gives the bits it has inside the batch
        const size_t b = M - 1;
        const void *one = dtype == DLLM_F32 ? static_cast<const void *>(&f32[b * ld]) : static_cast<const void *>(&f16[b * ld]);
        std::vector<float> p1(V);
        CHECK(dllm_token_readout_host(one, dtype, 1, V, V, tok2.data(), st2.data(), p1.data()) == DLLM_OK);
        CHECK(tok2[0] == tok[b] && bits(st2[0]) == bits(st[2 * b]) && bits(st2[1]) == bits(st[2 * b + 1]));
        CHECK(std::memcmp(p1.data(), &p[b * V], V * sizeof(float)) == 0);
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--exhaustive") == 0) return exhaustive();
    // EXP at its special points, and a strided sample of the range
    CHECK(bits(exp_le0(0.0f)) == 0x3f800000u && bits(exp_le0(-0.0f)) == 0x3f800000u);
    CHECK(bits(exp_le0(std::nanf(""))) == 0x7fc00000u);
    CHECK(bits(exp_le0(-std::numeric_limits<float>::infinity())) == 0u);
    CHECK(bits(exp_le0(std::nextafterf(-87.0f, -100.0f))) == 0u && bits(exp_le0(-1e30f)) == 0u);
    CHECK(exp_le0(-87.0f) >= 0x1p-126f);
    double worst = 0;
    for (uint64_t b = 0x80000000u; b <= 0xc2ae0000u; b += 4099) {
        const float d = from_bits(static_cast<uint32_t>(b));
        const float got = exp_le0(d);
        CHECK(got >= 0x1p-126f && got <= 1.0f);
        const double u = ulp_error(d);
        worst = u > worst ? u : worst;
    }
    std::printf("sampled max_ulp_error %.6f\n", worst);
    CHECK(worst <= static_cast<double>(dllm::token::kExpUlps));

    const size_t Vs[] = {1, 3, 4, 1023, 1025, 16383, 16384, 16385, 32773};
    for (size_t V : Vs)
        for (int dtype : {DLLM_F32, DLLM_F16}) {
            run(1, V, V, dtype, 0);
            run(3, V, V + 5, dtype, 0);
            for (int special = 1; special <= 3; ++special) run(2, V, V + 1, dtype, special);
        }
    std::vector<float> f(8);
    std::vector<int32_t> t(2);
    CHECK(dllm_token_readout_host(f.data(), DLLM_F32, 1, 0, 4, t.data(), f.data(), nullptr) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_token_readout_host(f.data(), DLLM_F32, 1, 4, 3, t.data(), f.data(), nullptr) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_token_readout_host(f.data(), DLLM_F32, 1, size_t(1) << 31, size_t(1) << 31, t.data(), f.data(), nullptr) ==
          DLLM_ERR_SHAPE_MISMATCH);
    CHECK(dllm_token_readout_host(f.data(), 7, 1, 4, 4, t.data(), f.data(), nullptr) == DLLM_ERR_UNSUPPORTED);
    CHECK(dllm_token_readout_host(nullptr, DLLM_F32, 0, 4, 4, nullptr, nullptr, nullptr) == DLLM_OK);
    CHECK(dllm_token_readout_host(nullptr, DLLM_F32, 1, 4, 4, t.data(), f.data(), nullptr) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_token_readout_host(f.data(), DLLM_F32, 1, 4, 4, nullptr, f.data(), nullptr) == DLLM_ERR_INVALID_PARAMS);
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
#else
int main() { return exhaustive(); }
#endif
