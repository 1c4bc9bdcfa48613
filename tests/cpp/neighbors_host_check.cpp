// neighbors_host_check.cpp -- a stand-alone driver of the host row-against-row entry points
// (dllm_neighbor_table_host / dllm_neighbor_rows_host, csrc/host_rules.cpp), meant to be compiled
// together with host_rules.cpp under the address and undefined-behaviour sanitizers and run on a
// CPU.  Every buffer is a heap allocation of exactly the size the header states, so a read or write
// past an end is caught; the values are checked for what needs no second implementation: the
// ranking order, the dropped self pair, the -1 / -inf tail, slice invariance, symmetry and the
// rejections.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

static uint32_t rng_state = 2463534242u;
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

// An exact-size, 8-byte aligned heap buffer for a pair table.
struct Table {
    void *p;
    size_t bytes;
    explicit Table(size_t rows) : p(nullptr), bytes(dllm_neighbor_table_bytes(rows)) { p = std::malloc(bytes ? bytes : 1); }
    ~Table() { std::free(p); }
    Table(const Table &) = delete;
    Table &operator=(const Table &) = delete;
};

static const float NINF = -std::numeric_limits<float>::infinity();

// The store against a block [q0, q0 + nq) of itself, with and without the self pair.
static void run(size_t rows, size_t dim, size_t q0, size_t nq, size_t k) {
    std::vector<uint8_t> codes(rows * dim);
    std::vector<float> scales(rows), zps(rows), sc(nq * k), sc2(nq * k);
    std::vector<int32_t> idx(nq * k), idx2(nq * k);
    for (auto &c : codes) c = static_cast<uint8_t>(rnd());
    for (size_t r = 0; r < rows; ++r) scales[r] = 0.01f + 0.01f * (rndf() + 1.0f), zps[r] = rndf();
    if (rows > 2) {   // rows 1 and 2 are copies of row 0: a tie, decided by the index
        for (size_t r = 1; r < 3; ++r) {
            std::memcpy(&codes[r * dim], &codes[0], dim);
            scales[r] = scales[0], zps[r] = zps[0];
        }
    }
    Table tab(rows);
    CHECK(dllm_neighbor_table_host(codes.data(), rows, dim, scales.data(), zps.data(), tab.p) == DLLM_OK);
    const uint8_t *qc = codes.data() + q0 * dim;
    const void *qt = static_cast<const uint8_t *>(tab.p) + dllm_neighbor_table_bytes(q0);
    CHECK(dllm_neighbor_rows_host(qc, qt, nq, codes.data(), tab.p, rows, dim, k, NINF, -1, idx.data(), sc.data()) == DLLM_OK);
    CHECK(dllm_neighbor_rows_host(qc, qt, nq, codes.data(), tab.p, rows, dim, k, NINF, static_cast<int64_t>(q0), idx2.data(),
                                  sc2.data()) == DLLM_OK);
    for (int self = 0; self < 2; ++self) {
        const std::vector<int32_t> &ix = self ? idx2 : idx;
        const std::vector<float> &s = self ? sc2 : sc;
        const size_t live = self ? rows - 1 : rows, top = k < live ? k : live;
        for (size_t j = 0; j < nq; ++j)
            for (size_t i = 0; i < k; ++i) {
                const int32_t id = ix[j * k + i];
                const float v = s[j * k + i];
                if (i >= top) {
                    CHECK(id == -1 && std::isinf(v) && v < 0);
                    continue;
                }
                CHECK(id >= 0 && static_cast<size_t>(id) < rows);
                CHECK(!self || static_cast<size_t>(id) != q0 + j);
                CHECK(std::fabs(v) <= 1.0f);
                if (i + 1 < top) {   // score descending, index ascending among equals
                    const float n = s[j * k + i + 1];
                    CHECK(v > n || (v == n && id < ix[j * k + i + 1]));
                }
            }
    }
    if (k >= rows) {
        for (size_t j = 0; j < nq; ++j) {   // a row against itself is 1 to the last f32 bit or two, and ranks first
            CHECK(std::fabs(sc[j * k] - 1.0f) <= 2.4e-7f);
            if (rows > 2 && q0 == 0 && j < 3) {   // the copies: the self pair is dropped, its duplicates stay, in index order
                CHECK(idx[j * k] == 0 && idx[j * k + 1] == 1 && idx[j * k + 2] == 2);
                CHECK(bits(sc[j * k]) == bits(sc[j * k + 1]) && bits(sc[j * k]) == bits(sc[j * k + 2]));
                const int32_t a = j == 0 ? 1 : 0, b = j == 2 ? 1 : 2;
                CHECK(idx2[j * k] == a && idx2[j * k + 1] == b);
            }
        }
        if (q0 == 0 && nq == rows) {   // symmetry of the bits
            std::vector<float> full(rows * rows);
            for (size_t j = 0; j < rows; ++j)
                for (size_t i = 0; i < rows; ++i) full[j * rows + idx[j * k + i]] = sc[j * k + i];
            for (size_t j = 0; j < rows; ++j)
                for (size_t t = 0; t < rows; ++t) CHECK(bits(full[j * rows + t]) == bits(full[t * rows + j]));
        }
    }
    if (rows > 4 && k >= rows && q0 == 0) {   // rows [2, rows) of the store on their own: the same bits, shifted indices
        const size_t a = 2, n = rows - a;
        Table t2(n);
        CHECK(dllm_neighbor_table_host(&codes[a * dim], n, dim, &scales[a], &zps[a], t2.p) == DLLM_OK);
        CHECK(std::memcmp(t2.p, static_cast<const uint8_t *>(tab.p) + dllm_neighbor_table_bytes(a), t2.bytes) == 0);
        CHECK(dllm_neighbor_rows_host(qc, qt, nq, &codes[a * dim], t2.p, n, dim, k, NINF, -1, idx2.data(), sc2.data()) ==
              DLLM_OK);
        for (size_t j = 0; j < nq; ++j)
            for (size_t i = 0; i < n; ++i) {
                const int32_t id = idx2[j * k + i] + static_cast<int32_t>(a);
                size_t at = 0;
                while (idx[j * k + at] != id) ++at;
                CHECK(bits(sc[j * k + at]) == bits(sc2[j * k + i]));
            }
    }
    if (rows > 1 && k >= rows) {   // a threshold equal to a score keeps it; the next float above drops it
        const float thr = sc[1];
        CHECK(dllm_neighbor_rows_host(qc, qt, 1, codes.data(), tab.p, rows, dim, k, thr, -1, idx2.data(), sc2.data()) == DLLM_OK);
        size_t kept = 0;
        while (kept < k && idx2[kept] >= 0) ++kept;
        size_t want = 0;
        for (size_t i = 0; i < rows; ++i) want += sc[i] >= thr;
        CHECK(kept == want && kept >= 2 && bits(sc2[1]) == bits(thr));
        CHECK(dllm_neighbor_rows_host(qc, qt, 1, codes.data(), tab.p, rows, dim, k, std::nextafter(thr, 2.0f), -1, idx2.data(),
                                      sc2.data()) == DLLM_OK);
        size_t kept2 = 0;
        while (kept2 < k && idx2[kept2] >= 0) ++kept2;
        size_t want2 = 0;
        for (size_t i = 0; i < rows; ++i) want2 += sc[i] > thr;
        CHECK(kept2 == want2 && kept2 < kept);
        CHECK(dllm_neighbor_rows_host(qc, qt, 1, codes.data(), tab.p, rows, dim, k, -NINF, -1, idx2.data(), sc2.data()) == DLLM_OK);
        for (size_t i = 0; i < k; ++i) CHECK(idx2[i] == -1 && sc2[i] == NINF);
    }
}

int main() {
    const size_t dims[] = {1, 3, 16, 63, 64, 65, 263, 768, 1025};
    for (size_t dim : dims) {
        run(1, dim, 0, 1, 1);
        run(7, dim, 0, 7, 7);
        run(7, dim, 2, 3, 9);     // k > rows, a block from the middle
        run(40, dim, 35, 5, 5);   // a block at the end
    }
    run(300, 32, 0, 2, 256);
    {   // an empty store: all tail
        std::vector<uint8_t> c(16);
        std::vector<int32_t> i(3);
        std::vector<float> s(3);
        Table q(1), none(0);
        std::vector<float> one(1, 0.5f);
        CHECK(dllm_neighbor_table_host(c.data(), 1, 16, one.data(), one.data(), q.p) == DLLM_OK);
        CHECK(dllm_neighbor_rows_host(c.data(), q.p, 1, nullptr, nullptr, 0, 16, 3, NINF, -1, i.data(), s.data()) == DLLM_OK);
        for (int n = 0; n < 3; ++n) CHECK(i[n] == -1 && s[n] == NINF);
    }
    std::vector<uint8_t> c(16);
    std::vector<int32_t> i(8);
    std::vector<float> f(8, 1.0f);
    Table t(2);
    CHECK(dllm_neighbor_table_host(c.data(), 2, 8, f.data(), f.data(), t.p) == DLLM_OK);
    auto call = [&](size_t nq, size_t rows, size_t dim, size_t k, float thr, int64_t base) {
        return dllm_neighbor_rows_host(c.data(), t.p, nq, c.data(), t.p, rows, dim, k, thr, base, i.data(), f.data());
    };
    CHECK(call(1, 2, 8, 0, 0.f, -1) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(1, 2, 8, 257, 0.f, -1) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(1, 2, 0, 1, 0.f, -1) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(1, 2, 65536, 1, 0.f, -1) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(1, size_t(1) << 31, 8, 1, 0.f, -1) == DLLM_ERR_SHAPE_MISMATCH);
    CHECK(call(1, 2, 8, 1, std::nanf(""), -1) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(1, 2, 8, 1, 0.f, -2) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(2, 2, 8, 1, 0.f, 1) == DLLM_ERR_INVALID_PARAMS);
    CHECK(call(1, 2, 8, 1, 0.f, 1) == DLLM_OK);
    CHECK(dllm_neighbor_rows_host(nullptr, nullptr, 0, nullptr, nullptr, 2, 8, 1, 0.f, -1, nullptr, nullptr) == DLLM_OK);
    CHECK(dllm_neighbor_rows_host(nullptr, t.p, 1, c.data(), t.p, 2, 8, 1, 0.f, -1, i.data(), f.data()) == DLLM_ERR_INVALID_PARAMS);
    CHECK(dllm_neighbor_table_host(nullptr, 1, 8, f.data(), f.data(), t.p) == DLLM_ERR_INVALID_PARAMS);
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
