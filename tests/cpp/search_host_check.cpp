// search_host_check.cpp -- a stand-alone driver of the host search entry points
// (dllm_search_table_host / dllm_search_vectors_host, csrc/host_rules.cpp), meant to be compiled
// together with host_rules.cpp under the address and undefined-behaviour sanitizers and run on a
// CPU.  Every buffer is a heap allocation of exactly the size the header states, so a read or write
// past an end is caught; the values are checked for what needs no second implementation: the
// ranking order, slice invariance, the -1 / -inf tail and the rejections.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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

static uint32_t rng_state = 12345u;
static uint32_t rnd() {   // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}
static float rndf() { return static_cast<float>(rnd() >> 8) / 8388608.0f - 1.0f; }

static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

static void run(size_t rows, size_t dim, size_t nq, size_t k) {
    std::vector<uint8_t> codes(rows * dim);
    std::vector<float> scales(rows), zps(rows), table(2 * rows), Q(nq * dim), sc(nq * k), sc2(nq * k);
    std::vector<int32_t> idx(nq * k), idx2(nq * k);
    for (auto &c : codes) c = static_cast<uint8_t>(rnd());
    for (size_t r = 0; r < rows; ++r) scales[r] = 0.01f + 0.01f * (rndf() + 1.0f), zps[r] = rndf();
    for (auto &q : Q) q = rndf();
    if (rows > 2) {   // rows 1 and 2 are copies of row 0: a tie, decided by the index
        for (size_t r = 1; r < 3; ++r) {
            std::memcpy(&codes[r * dim], &codes[0], dim);
            scales[r] = scales[0], zps[r] = zps[0];
        }
    }
    CHECK(dllm_search_table_host(codes.data(), rows, dim, scales.data(), zps.data(), table.data()) == DLLM_OK);
    CHECK(dllm_search_vectors_host(Q.data(), nq, codes.data(), table.data(), rows, dim, k, idx.data(), sc.data()) ==
          DLLM_OK);
    const size_t top = k < rows ? k : rows;
    for (size_t j = 0; j < nq; ++j) {
        for (size_t i = 0; i < k; ++i) {
            const int32_t id = idx[j * k + i];
            const float s = sc[j * k + i];
            if (i >= top) {
                CHECK(id == -1 && std::isinf(s) && s < 0);
                continue;
            }
            CHECK(id >= 0 && static_cast<size_t>(id) < rows);
            CHECK(std::fabs(s) <= 1.0f + 1e-4f);
            if (i + 1 < top) {   // score descending, index ascending among equals
                const float n = sc[j * k + i + 1];
                CHECK(s > n || (s == n && id < idx[j * k + i + 1]));
            }
        }
        if (rows > 2 && k >= rows) {   // the three copies score the same bits and stand in index order
            size_t at = 0;
            while (idx[j * k + at] != 0) ++at;
            CHECK(at + 2 < top && idx[j * k + at + 1] == 1 && idx[j * k + at + 2] == 2);
            CHECK(bits(sc[j * k + at]) == bits(sc[j * k + at + 1]) && bits(sc[j * k + at]) == bits(sc[j * k + at + 2]));
        }
    }
    if (rows > 4 && k >= rows) {   // rows [2, rows) on their own: the same bits for the same rows
        const size_t a = 2, n = rows - a;
        std::vector<float> t2(2 * n);
        CHECK(dllm_search_table_host(&codes[a * dim], n, dim, &scales[a], &zps[a], t2.data()) == DLLM_OK);
        CHECK(std::memcmp(t2.data(), &table[2 * a], 2 * n * sizeof(float)) == 0);
        CHECK(dllm_search_vectors_host(Q.data(), nq, &codes[a * dim], t2.data(), n, dim, k, idx2.data(), sc2.data()) ==
              DLLM_OK);
        for (size_t j = 0; j < nq; ++j)
            for (size_t i = 0; i < n; ++i) {
                const int32_t id = idx2[j * k + i] + static_cast<int32_t>(a);
                size_t at = 0;
                while (idx[j * k + at] != id) ++at;
                CHECK(bits(sc[j * k + at]) == bits(sc2[j * k + i]));
            }
    }
}

int main() {
    const size_t dims[] = {1, 3, 4, 64, 255, 256, 263, 768, 1025};
    for (size_t dim : dims) {
        run(1, dim, 1, 1);
        run(7, dim, 3, 7);
        run(7, dim, 2, 9);     // k > rows
        run(40, dim, 2, 5);
    }
    run(0, 16, 2, 3);          // an empty store: all tail
    run(300, 32, 1, 256);
    std::vector<float> f(8);
    std::vector<uint8_t> c(8);
    std::vector<int32_t> i(8);
    CHECK(dllm_search_vectors_host(f.data(), 1, c.data(), f.data(), 1, 8, 0, i.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_search_vectors_host(f.data(), 1, c.data(), f.data(), 1, 8, 257, i.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_search_vectors_host(f.data(), 1, c.data(), f.data(), 1, 0, 1, i.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_search_vectors_host(nullptr, 1, c.data(), f.data(), 1, 8, 1, i.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_search_vectors_host(f.data(), 1, c.data(), f.data(), size_t(1) << 31, 8, 1, i.data(), f.data()) ==
          DLLM_ERR_SHAPE_MISMATCH);
    CHECK(dllm_search_vectors_host(nullptr, 0, nullptr, nullptr, 1, 8, 1, nullptr, nullptr) == DLLM_OK);
    CHECK(dllm_search_table_host(nullptr, 1, 8, f.data(), f.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
