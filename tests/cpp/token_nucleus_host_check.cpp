// token_nucleus_host_check.cpp -- a stand-alone driver (its own main) of the host side of top-p / min-p
// sampling: dllm_token_sample_ex_host (csrc/host_rules.cpp) on exact-size heap buffers, meant to be
// compiled with host_rules.cpp under the address and undefined-behaviour sanitizers: a read or write
// past an end is caught.  The values are checked for what needs no second implementation: with both
// masks off the outputs are dllm_token_sample_host's; the token lies in the row and at or above tau;
// tau is one of the row's values and never below the top-k threshold; the kept mass reaches the share
// top_p and, where top-p set tau, does not without the elements at tau; where min-p set it, an element
// at tau has a weight of at least mfix; a smaller top_p and a larger min_p never lower tau; padding is
// never read; the degenerate rows; the rejections.
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
#include "token_nucleus_rule.hpp"

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

static uint16_t half_of(float v) {   // finite values used here are exactly representable: k / 64, |k| <= 1024
    if (v != v) return 0x7e00;
    if (std::isinf(v)) return v > 0 ? 0x7c00 : 0xfc00;
    const uint32_t b = bits(v);
    if ((b & 0x7fffffffu) == 0) return static_cast<uint16_t>(b >> 16);
    const int e = static_cast<int>((b >> 23) & 0xff) - 127 + 15;
    return static_cast<uint16_t>(((b >> 16) & 0x8000u) | (static_cast<uint32_t>(e) << 10) | ((b >> 13) & 0x3ffu));
}

struct Buffers {
    std::vector<float> x, f32;
    std::vector<uint16_t> f16;
    const void *logits;
};

static Buffers make(size_t M, size_t V, size_t ld, int dtype, int special) {
    const float inf = std::numeric_limits<float>::infinity();
    Buffers B;
    B.x.resize(M * V);
    for (auto &v : B.x) v = std::floor(rndf() * 512.0f) / 64.0f;    // multiples of 1/64 in [-8, 8): exact in f16
    if (special == 1 && V > 2) B.x[V / 2] = std::nanf("");
    if (special == 2)
        for (size_t i = 0; i < V; ++i) B.x[i] = -inf;
    if (special == 3) B.x[V - 1] = inf;
    const size_t total = (M - 1) * ld + V;                          // the last row has V elements, not ld
    B.f32.resize(dtype == DLLM_F32 ? total : 0);
    B.f16.resize(dtype == DLLM_F16 ? total : 0);
    for (size_t i = 0; i < total; ++i) {
        const size_t b = i / ld, c = i % ld;
        const float v = c < V ? B.x[b * V + c] : (c % 2 ? inf : std::nanf(""));
        if (dtype == DLLM_F32)
            B.f32[i] = v;
        else
            B.f16[i] = half_of(v);
    }
    B.logits = dtype == DLLM_F32 ? static_cast<const void *>(B.f32.data()) : static_cast<const void *>(B.f16.data());
    return B;
}

static void run(size_t M, size_t V, size_t ld, int dtype, float T, size_t top_k, float top_p, float min_p, int special) {
    const float inf = std::numeric_limits<float>::infinity();
    const Buffers B = make(M, V, ld, dtype, special);
    std::vector<int32_t> tok(M), tok3(M);
    std::vector<float> st(4 * M), st3(3 * M), lo(4 * M), hi(4 * M);
    CHECK(dllm_token_sample_ex_host(B.logits, dtype, M, V, ld, T, top_k, top_p, min_p, nullptr, 77, ~uint64_t(0), tok.data(),
                                    st.data()) == DLLM_OK);
    if (top_p == 1.0f && min_p == 0.0f) {
        CHECK(dllm_token_sample_host(B.logits, dtype, M, V, ld, T, top_k, nullptr, 77, ~uint64_t(0), tok3.data(), st3.data()) ==
              DLLM_OK);
        for (size_t b = 0; b < M; ++b)
            CHECK(tok[b] == tok3[b] && std::memcmp(&st[4 * b], &st3[3 * b], 12) == 0);
    }
    // a smaller top_p and a larger min_p: the threshold never falls
    CHECK(dllm_token_sample_ex_host(B.logits, dtype, M, V, ld, T, top_k, top_p * 0.5f, min_p, nullptr, 77, 0, tok3.data(),
                                    lo.data()) == DLLM_OK);
    CHECK(dllm_token_sample_ex_host(B.logits, dtype, M, V, ld, T, top_k, top_p, 0.5f * (min_p + 1.0f), nullptr, 77, 0,
                                    tok3.data(), hi.data()) == DLLM_OK);
    const float r = 1.0f / T;
    const uint64_t pfix = dllm::token::nucleus_pfix(top_p), mfix = dllm::token::nucleus_mfix(min_p);
    for (size_t b = 0; b < M; ++b) {
        const float *s = &st[4 * b];
        const bool plain = special == 0 || b > 0 || (special == 1 && V <= 2);
        if (!plain) {
            CHECK(tok[b] == -1);
            for (int i = 0; i < 4; ++i) CHECK(bits(s[i]) == 0x7fc00000u);
            continue;
        }
        std::vector<float> y(V);
        float m = -inf;
        for (size_t i = 0; i < V; ++i) {
            y[i] = B.x[b * V + i] * r;
            m = y[i] > m ? y[i] : m;
        }
        float tau_k = -inf;
        if (top_k > 0 && top_k < V) {
            std::vector<float> sorted(y);
            std::sort(sorted.begin(), sorted.end(), std::greater<float>());
            tau_k = sorted[top_k - 1];
        }
        const float tau = s[3];
        CHECK(bits(s[0]) == bits(m + 0.0f) && s[1] >= 1.0f && s[1] <= static_cast<float>(V) && s[2] > 0.0f && s[2] <= 1.0f);
        CHECK(tau >= tau_k && tau <= m && lo[4 * b + 3] >= tau && hi[4 * b + 3] >= tau);
        CHECK(tok[b] >= 0 && static_cast<size_t>(tok[b]) < V && y[static_cast<size_t>(tok[b])] >= tau);
        if (tau == -inf) {
            CHECK(top_p == 1.0f && min_p == 0.0f && tau_k == -inf);
            continue;
        }
        // the integer sums around tau: T, the mass at or above tau, the mass strictly above it
        uint64_t Tsum = 0, ge = 0, gt = 0;
        bool present = false;
        for (size_t i = 0; i < V; ++i) {
            const uint64_t W = y[i] >= tau_k ? dllm::token::nucleus_weight(exp_le0(y[i] - m)) : 0;
            Tsum += W;
            if (y[i] >= tau) ge += W;
            if (y[i] > tau) gt += W;
            present |= y[i] == tau;
        }
        CHECK(present);
        if (top_p != 1.0f) CHECK(dllm::token::nucleus_reaches(ge, pfix, Tsum));
        // tau is the largest of three: were it raised past its ties, one of the masks would object
        const bool p_holds = top_p != 1.0f && !dllm::token::nucleus_reaches(gt, pfix, Tsum);
        bool m_holds = false;
        if (min_p != 0.0f)
            for (size_t i = 0; i < V; ++i)
                m_holds |= y[i] == tau && y[i] >= tau_k && dllm::token::nucleus_weight(exp_le0(y[i] - m)) >= mfix;
        CHECK(p_holds || m_holds || tau == tau_k);
    }
}

int main() {
    const size_t Vs[] = {1, 3, 4, 1023, 1025, 16384, 16385, 32773};
    const float pred1 = std::nextafter(1.0f, 0.0f);
    const float masks[][2] = {{1.0f, 0.0f},  {0x1p-30f, 0.0f}, {0.5f, 0.0f},  {0.9f, 0.0f},     {pred1, 0.0f},
                              {1.0f, 0x1p-33f}, {1.0f, 0.05f}, {1.0f, 1.0f}, {0.9f, 0.05f}};
    for (size_t V : Vs)
        for (int dtype : {DLLM_F32, DLLM_F16}) {
            for (const auto &pm : masks)
                for (size_t k : {size_t(0), size_t(50)}) {
                    run(1, V, V, dtype, 1.0f, k, pm[0], pm[1], 0);
                    run(3, V, V + 5, dtype, 0.7f, k, pm[0], pm[1], 0);
                }
            for (int special = 1; special <= 3; ++special) run(2, V, V + 1, dtype, 0.5f, 2, 0.9f, 0.05f, special);
        }
    std::vector<float> f(8, 0.0f);
    std::vector<int32_t> t(2);
    const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
    auto call = [&](const void *l, int dtype, size_t M, size_t V, size_t ld, float T, float top_p, float min_p, int32_t *tk,
                    float *s) { return dllm_token_sample_ex_host(l, dtype, M, V, ld, T, 0, top_p, min_p, nullptr, 0, 0, tk, s); };
    CHECK(call(f.data(), DLLM_F32, 1, 0, 4, 1.0f, 0.9f, 0.0f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, 4, 3, 1.0f, 0.9f, 0.0f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, size_t(1) << 31, size_t(1) << 31, 1.0f, 0.9f, 0.0f, t.data(), f.data()) ==
          DLLM_ERR_SHAPE_MISMATCH);
    CHECK(call(f.data(), 7, 1, 4, 4, 1.0f, 0.9f, 0.0f, t.data(), f.data()) == DLLM_ERR_UNSUPPORTED);
    CHECK(call(f.data(), DLLM_F32, 1, 4, 4, 0.0f, 0.9f, 0.0f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    for (float p : {0.0f, -1.0f, nan, inf, std::nextafter(1.0f, 2.0f)})
        CHECK(call(f.data(), DLLM_F32, 1, 4, 4, 1.0f, p, 0.0f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    for (float p : {-0x1p-100f, nan, inf, std::nextafter(1.0f, 2.0f)})
        CHECK(call(f.data(), DLLM_F32, 1, 4, 4, 1.0f, 0.9f, p, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), 7, 1, 4, 4, 1.0f, 2.0f, 2.0f, t.data(), f.data()) == DLLM_ERR_UNSUPPORTED);
    CHECK(call(nullptr, DLLM_F32, 0, 4, 4, 1.0f, 0.9f, 0.05f, nullptr, nullptr) == DLLM_OK);
    CHECK(call(nullptr, DLLM_F32, 0, 4, 4, 1.0f, 0.0f, 0.05f, nullptr, nullptr) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(nullptr, DLLM_F32, 1, 4, 4, 1.0f, 0.9f, 0.05f, t.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, 4, 4, 1.0f, 0.9f, 0.05f, nullptr, f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(f.data(), DLLM_F32, 1, 4, 4, 1.0f, 0.9f, 0.05f, t.data(), nullptr) == DLLM_ERR_INVALID_PARAMS);
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
