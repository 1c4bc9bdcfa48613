// token_sample_host_check.cpp -- a stand-alone driver (its own main) of token sampling's host side:
// dllm_token_sample_host (csrc/host_rules.cpp) on exact-size heap buffers, meant to be compiled with
// host_rules.cpp under the address and undefined-behaviour sanitizers: a read or write past an end is
// caught.  The values are checked for what needs no second implementation: the token lies in the row
// and survives the mask, Z >= 1, p_token = EXP(y_tok - m) / Z <= 1, {m, Z} do not depend on the
// uniforms, the extreme uniforms give the first and the last live element, padding is never read,
// a row on its own gives the bits it has inside a batch, the degenerate rows, the rejections.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

#include "dllm_quant.h"
#include "token_exp.hpp"

using dllm::token::exp_le0;

static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

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
static uint16_t half_of(float v) {
    if (v != v) return 0x7e00;
    if (std::isinf(v)) return v > 0 ? 0x7c00 : 0xfc00;
    return to_half(v);
}

static const float kLast = 1.0f - 0x1p-24f;

static void run(size_t M, size_t V, size_t ld, int dtype, float T, size_t top_k, int special) {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> x(M * V);
    for (auto &v : x) v = std::floor(rndf() * 512.0f) / 64.0f;      // multiples of 1/64 in [-8, 8): exact in f16
    if (special == 1 && V > 2) x[V / 2] = std::nanf("");
    if (special == 2)
        for (size_t i = 0; i < V; ++i) x[i] = -inf;
    if (special == 3) x[V - 1] = inf;
    // exact-size buffers: the last row has V elements, not ld; padding holds NaN and +inf
    const size_t total = (M - 1) * ld + V;
    std::vector<float> f32(dtype == DLLM_F32 ? total : 0);
    std::vector<uint16_t> f16(dtype == DLLM_F16 ? total : 0);
    for (size_t i = 0; i < total; ++i) {
        const size_t b = i / ld, c = i % ld;
        const float v = c < V ? x[b * V + c] : (c % 2 ? inf : std::nanf(""));
        if (dtype == DLLM_F32)
            f32[i] = v;
        else
            f16[i] = half_of(v);
    }
    const void *logits = dtype == DLLM_F32 ? static_cast<const void *>(f32.data()) : static_cast<const void *>(f16.data());
    std::vector<int32_t> tok(M), tok0(M), tok1(M);
    std::vector<float> st(3 * M), st0(3 * M), st1(3 * M), u0(3 * M, 0.0f), u1(3 * M, kLast);
    CHECK(dllm_token_sample_host(logits, dtype, M, V, ld, T, top_k, nullptr, 77, ~uint64_t(0), tok.data(), st.data()) == DLLM_OK);
    CHECK(dllm_token_sample_host(logits, dtype, M, V, ld, T, top_k, u0.data(), 0, 0, tok0.data(), st0.data()) == DLLM_OK);
    CHECK(dllm_token_sample_host(logits, dtype, M, V, ld, T, top_k, u1.data(), 0, 0, tok1.data(), st1.data()) == DLLM_OK);
    const float r = 1.0f / T;
    for (size_t b = 0; b < M; ++b) {
        const bool plain = special == 0 || b > 0 || (special == 1 && V <= 2);
        if (!plain) {
            CHECK(tok[b] == -1 && bits(st[3 * b]) == 0x7fc00000u && bits(st[3 * b + 1]) == 0x7fc00000u &&
                  bits(st[3 * b + 2]) == 0x7fc00000u);
            continue;
        }
        std::vector<float> y(V);
        for (size_t i = 0; i < V; ++i) y[i] = x[b * V + i] * r;
        float tau = -inf;
        if (top_k > 0 && top_k < V) {
            std::vector<float> s(y);
            std::sort(s.begin(), s.end(), std::greater<float>());
            tau = s[top_k - 1];
        }
        size_t first = V, last = V;
        float mx = -inf;
        for (size_t i = 0; i < V; ++i) {
            if (!(y[i] >= tau)) continue;
            mx = y[i] > mx ? y[i] : mx;
        }
        for (size_t i = 0; i < V; ++i)
            if (y[i] >= tau && exp_le0(y[i] - mx) > 0.0f) last = i, first = first == V ? i : first;
        const float m = st[3 * b], Z = st[3 * b + 1];
        CHECK(bits(m) == bits(mx + 0.0f) && Z >= 1.0f && Z <= static_cast<float>(V));
        for (const auto *t : {&tok, &tok0, &tok1}) {
            const int32_t k = (*t)[b];
            CHECK(k >= 0 && static_cast<size_t>(k) < V && y[static_cast<size_t>(k)] >= tau);
        }
        CHECK(bits(st[3 * b + 2]) == bits(exp_le0(y[static_cast<size_t>(tok[b])] - m) / Z) && st[3 * b + 2] <= 1.0f);
        CHECK(bits(st0[3 * b]) == bits(m) && bits(st0[3 * b + 1]) == bits(Z) && bits(st1[3 * b + 1]) == bits(Z));
        // every chunk maximum is within 16 / T of the row maximum here, so no chunk's weight is +0: the
        // extreme uniforms reach the first live element of chunk 0's lane 0 ... and the row's last live one
        if (V <= 4) CHECK(static_cast<size_t>(tok0[b]) == first);
        CHECK(static_cast<size_t>(tok1[b]) <= last);
    }
    if (M > 1) {   // a row on its own, at its own counter, gives the bits it has inside the batch
        const size_t b = M - 1;
        const void *one = dtype == DLLM_F32 ? static_cast<const void *>(&f32[b * ld]) : static_cast<const void *>(&f16[b * ld]);
        int32_t t1;
        float s1[3];
        CHECK(dllm_token_sample_host(one, dtype, 1, V, V, T, top_k, nullptr, 77, ~uint64_t(0) + b, &t1, s1) == DLLM_OK);
        CHECK(t1 == tok[b] && std::memcmp(s1, &st[3 * b], sizeof(s1)) == 0);
    }
}

int main() {
    const size_t Vs[] = {1, 3, 4, 1023, 1025, 16383, 16384, 16385, 32773};
    for (size_t V : Vs)
        for (int dtype : {DLLM_F32, DLLM_F16}) {
            const size_t ks[] = {0, 1, 2, 50, V - 1, V, V + 7};
            for (size_t k : ks) {
                run(1, V, V, dtype, 1.0f, k, 0);
                run(3, V, V + 5, dtype, 0.7f, k, 0);
            }
            for (int special = 1; special <= 3; ++special) run(2, V, V + 1, dtype, 0.5f, 2, special);
        }
    std::vector<float> f(8, 0.0f);
    std::vector<int32_t> t(2);
    const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
    auto call = [&](const void *l, int dtype, size_t M, size_t V, size_t ld, float T, int32_t *tk, float *s) {
        return dllm_token_sample_host(l, dtype, M, V, ld, T, 0, nullptr, 0, 0, tk, s);
    };
    CHECK(call(f.data(), DLLM_F32, 1, 0, 4, 1.0f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, 4, 3, 1.0f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, size_t(1) << 31, size_t(1) << 31, 1.0f, t.data(), f.data()) == DLLM_ERR_SHAPE_MISMATCH);
    CHECK(call(f.data(), 7, 1, 4, 4, 1.0f, t.data(), f.data()) == DLLM_ERR_UNSUPPORTED);
    for (float T : {0.0f, -1.0f, nan, inf, 1e-45f}) CHECK(call(f.data(), DLLM_F32, 1, 4, 4, T, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), 7, 1, 4, 4, 0.0f, t.data(), f.data()) == DLLM_ERR_UNSUPPORTED);
    CHECK(call(nullptr, DLLM_F32, 0, 4, 4, 1.0f, nullptr, nullptr) == DLLM_OK);
    CHECK(call(nullptr, DLLM_F32, 1, 4, 4, 1.0f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, 4, 4, 1.0f, nullptr, f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, 4, 4, 1.0f, t.data(), nullptr) == DLLM_ERR_INVALID_PARAMS);
    // out-of-range and NaN uniforms: no pick, m and Z still written
    for (float v : {1.0f, nan}) {
        const float u[3] = {0.5f, v, 0.5f};
        float s[3];
        CHECK(dllm_token_sample_host(f.data(), DLLM_F32, 1, 8, 8, 1.0f, 0, u, 0, 0, t.data(), s) == DLLM_OK);
        CHECK(t[0] == -1 && s[0] == 0.0f && s[1] == 8.0f && bits(s[2]) == 0x7fc00000u);
    }
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
