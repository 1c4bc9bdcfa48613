// dedup_host_check.cpp -- a stand-alone driver (its own main) of the host dedup entry points
// (dllm_hash_rows_host, dllm_dedup_table_init_host, dllm_dedup_rows_host, dllm_gather_rows_host,
// csrc/host_rules.cpp), meant to be compiled together with host_rules.cpp under the address and
// undefined-behaviour sanitizers and run on a CPU.  Every buffer is a heap allocation of exactly the
// size the header states, so a read or write past an end is caught.  The values are checked against
// forms that need no second implementation of the entry: the hash as a power-weighted sum, the filter
// by a quadratic search for an earlier equal hash, the full-table flag with a dishonest base.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dedup_rule.hpp"
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

static size_t table_bytes(size_t slots) { return dllm::dedup::table_words(slots) * 8; }

static void run_hash(size_t rows, size_t dim, size_t ld) {
    std::vector<uint8_t> codes(rows ? (rows - 1) * ld + dim : 0);   // the last row ends at its dim-th byte
    for (auto &c : codes) c = static_cast<uint8_t>(rnd());
    std::vector<uint64_t> h(rows);
    CHECK(dllm_hash_rows_host(codes.data(), rows, dim, ld, h.data()) == DLLM_OK);
    for (size_t r = 0; r < rows; ++r) {
        uint64_t want = 0, w = 1;
        for (size_t i = dim; i-- > 0;) {
            want += codes[r * ld + i] * w;
            w *= 31u;
        }
        CHECK(h[r] == want);
    }
}

// One table, `calls` batches of `rows` hashes drawn from a pool of `pool` values.
static void run_filter(size_t rows, size_t calls, size_t pool, bool with_table) {
    const size_t total = rows * calls;
    size_t slots = 2;
    while (slots < 2 * total) slots <<= 1;
    std::vector<uint8_t> table(with_table ? table_bytes(slots) : 0);
    if (with_table) CHECK(dllm_dedup_table_init_host(table.data(), slots) == DLLM_OK);
    std::vector<uint64_t> all;
    for (size_t c = 0; c < calls; ++c) {
        std::vector<uint64_t> h(rows), first(rows);
        std::vector<uint8_t> keep(rows);
        std::vector<int32_t> kept(rows);
        uint32_t n = 77;
        for (auto &x : h) {
            const uint32_t v = rnd() % pool;
            x = v == 0 ? ~uint64_t(0) : (v == 1 ? 0 : v * 0x9E3779B97F4A7C15ull);   // the reserved key and 0 among them
        }
        const uint64_t base = with_table ? c * rows : 5;
        if (!with_table) all.clear();
        CHECK(dllm_dedup_rows_host(h.data(), rows, base, with_table ? table.data() : nullptr, slots, keep.data(),
                                   first.data(), kept.data(), &n) == DLLM_OK);
        const size_t before = all.size();
        uint32_t cnt = 0;
        for (size_t r = 0; r < rows; ++r) {
            size_t f = 0;
            while (f < all.size() && all[f] != h[r]) ++f;
            const uint64_t seq0 = with_table ? 0 : base;
            CHECK(keep[r] == (f == all.size() ? 1 : 0));
            CHECK(first[r] == seq0 + f);
            if (keep[r]) CHECK(kept[cnt] == static_cast<int32_t>(r));
            cnt += keep[r];
            all.push_back(h[r]);
        }
        (void)before;
        CHECK(n == cnt);
        for (size_t i = cnt; i < rows; ++i) CHECK(kept[i] == -1);
    }
    if (with_table) {
        uint64_t w[2];
        std::memcpy(w, table.data(), 16);
        CHECK(w[0] == 0);
        size_t distinct = 0;
        for (size_t i = 0; i < all.size(); ++i) {
            size_t f = 0;
            while (all[f] != all[i]) ++f;
            distinct += f == i;
        }
        CHECK(w[1] == distinct);
    }
}

static void run_full_table() {
    // A dishonest base: 8 slots take 4 honest rows; offering 12 distinct hashes 4 at a time, each call
    // claiming base = 0, fills the table.  The flag goes up, the rows without a slot come back dropped
    // with first = 2^64 - 1, and nothing is written out of bounds.
    const size_t slots = 8;
    std::vector<uint8_t> table(table_bytes(slots));
    CHECK(dllm_dedup_table_init_host(table.data(), slots) == DLLM_OK);
    size_t kept_total = 0;
    for (int c = 0; c < 3; ++c) {
        std::vector<uint64_t> h(4), first(4);
        std::vector<uint8_t> keep(4);
        std::vector<int32_t> kept(4);
        uint32_t n = 0;
        for (size_t r = 0; r < 4; ++r) h[r] = 1000 + 4 * c + r;
        CHECK(dllm_dedup_rows_host(h.data(), 4, 0, table.data(), slots, keep.data(), first.data(), kept.data(), &n) == DLLM_OK);
        kept_total += n;
        for (size_t r = 0; r < 4; ++r) CHECK(keep[r] == 1 || first[r] == ~uint64_t(0));
    }
    uint64_t w[2];
    std::memcpy(w, table.data(), 16);
    CHECK(kept_total == 8 && w[0] == 1 && w[1] == 8);
}

static void run_gather(size_t rows, size_t dim, size_t ld) {
    std::vector<uint8_t> codes((rows - 1) * ld + dim);
    for (auto &c : codes) c = static_cast<uint8_t>(rnd());
    std::vector<int32_t> kept(rows, -1);
    uint32_t n = 0;
    for (size_t r = 0; r < rows; ++r)
        if (rnd() & 1) kept[n++] = static_cast<int32_t>(r);
    std::vector<uint8_t> out(rows * dim, 0xA5);
    CHECK(dllm_gather_rows_host(codes.data(), dim, ld, kept.data(), &n, out.data(), dim) == DLLM_OK);
    for (size_t i = 0; i < rows; ++i)
        for (size_t d = 0; d < dim; ++d) CHECK(out[i * dim + d] == (i < n ? codes[kept[i] * ld + d] : 0xA5));
}

int main() {
    const size_t dims[] = {1, 3, 15, 16, 17, 64, 255, 769, 4097, 65535};
    for (size_t dim : dims) {
        run_hash(3, dim, dim);
        run_hash(2, dim, dim + 5);
    }
    run_hash(0, 8, 8);
    run_hash(1025, 7, 7);
    for (int with_table = 0; with_table < 2; ++with_table) {
        run_filter(1, 1, 2, with_table);
        run_filter(65, 3, 40, with_table);
        run_filter(300, 3, 1000000, with_table);   // hardly a duplicate
        run_filter(300, 2, 3, with_table);         // hardly anything else
    }
    run_full_table();
    run_gather(1, 1, 1);
    run_gather(9, 17, 17);
    run_gather(40, 769, 800);

    std::vector<uint8_t> c(64), k(8), t(table_bytes(8));
    std::vector<uint64_t> h(8), f(8);
    std::vector<int32_t> kr(8);
    uint32_t n = 0;
    const int INV = DLLM_ERR_INVALID_PARAMS;
    CHECK(dllm_hash_rows_host(c.data(), 1, 0, 8, h.data()) == INV);
    CHECK(dllm_hash_rows_host(c.data(), 1, 65536, 65536, h.data()) == INV);
    CHECK(dllm_hash_rows_host(c.data(), 1, 8, 7, h.data()) == INV);
    CHECK(dllm_hash_rows_host(nullptr, 1, 8, 8, h.data()) == INV);
    CHECK(dllm_hash_rows_host(c.data(), size_t(1) << 31, 8, 8, h.data()) == DLLM_ERR_SHAPE_MISMATCH);
    CHECK(dllm_hash_rows_host(nullptr, 0, 8, 8, nullptr) == DLLM_OK);
    CHECK(dllm_dedup_table_init_host(t.data(), 6) == INV);
    CHECK(dllm_dedup_table_init_host(nullptr, 8) == INV);
    CHECK(dllm_dedup_table_init_host(t.data(), 8) == DLLM_OK);
    CHECK(dllm_dedup_rows_host(h.data(), 4, 0, t.data(), 6, k.data(), f.data(), kr.data(), &n) == INV);
    CHECK(dllm_dedup_rows_host(h.data(), 5, 0, t.data(), 8, k.data(), f.data(), kr.data(), &n) == INV);
    CHECK(dllm_dedup_rows_host(h.data(), 2, 3, t.data(), 8, k.data(), f.data(), kr.data(), &n) == INV);
    CHECK(dllm_dedup_rows_host(nullptr, 4, 0, t.data(), 8, k.data(), f.data(), kr.data(), &n) == INV);
    CHECK(dllm_dedup_rows_host(h.data(), 4, 0, t.data(), 8, k.data(), f.data(), kr.data(), nullptr) == INV);
    CHECK(dllm_dedup_rows_host(nullptr, 0, 4, t.data(), 8, nullptr, nullptr, nullptr, nullptr) == DLLM_OK);
    CHECK(dllm_dedup_rows_host(h.data(), 4, 0, t.data(), 8, k.data(), f.data(), kr.data(), &n) == DLLM_OK);
    CHECK(dllm_gather_rows_host(c.data(), 8, 8, kr.data(), &n, c.data(), 7) == INV);
    CHECK(dllm_gather_rows_host(c.data(), 8, 8, nullptr, &n, c.data(), 8) == INV);
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
