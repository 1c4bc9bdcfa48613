// host_rules.cpp -- the rules of include/dllm_quant.h 8g - 8l in plain C++: the search, neighbour,
// token and dedup *_host entry points, the mirrors of search.hip, neighbors.hip, token.hip and dedup.hip
// that the tests hold the kernels against.  No HIP: this file, error.cpp and the rule headers build
// with any C++17 compiler (-ffp-contract=off), which is how tests/cpp/*_host_check.cpp run them under
// the sanitizers.  The argument checks are the rule headers' functions, the same calls as the device
// entry points make.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "dedup_rule.hpp"
#include "dllm_quant.h"
#include "error.hpp"
#include "neighbor_rule.hpp"
#include "search_rule.hpp"
#include "token_args.hpp"
#include "token_exp.hpp"
#include "token_nucleus_rule.hpp"
#include "token_sample_rule.hpp"

namespace {

using dllm::kTokChunk;
using dllm::search::search_key;

// ---- the search rule in plain C++ (include/dllm_quant.h 8g; csrc/search.hip is the device form) ----

// Strand sum of x[d] * y[d]: element d to strand (d / 4) % 64, each strand from +0 over its d
// ascending with one fmaf per element, the 64 partials by the tree a[i] = a[i] + a[i ^ m].
// y: the codes (as float), x itself (y_self), or 1.0f when both are null.
float strand_sum(const float *x, const uint8_t *codes, bool y_self, size_t dim) {
    float a[64], b[64];
    for (int i = 0; i < 64; ++i) a[i] = 0.0f;
    for (size_t d = 0; d < dim; ++d) {
        const float y = codes ? static_cast<float>(codes[d]) : (y_self ? x[d] : 1.0f);
        float &acc = a[(d / 4) % 64];
        acc = std::fmaf(x[d], y, acc);
    }
    for (int m = 32; m > 0; m >>= 1) {
        for (int i = 0; i < 64; ++i) b[i] = a[i] + a[i ^ m];
        std::memcpy(a, b, sizeof(a));
    }
    return a[0];
}

// ---- the token readout rule in plain C++ (include/dllm_quant.h 8h; csrc/token.hip is the device form) ----

float half_bits_to_float(uint16_t h) {   // exact widening of an IEEE binary16
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, em = h & 0x7fffu;
    uint32_t b;
    if (em >= 0x7c00u) {
        b = sign | 0x7f800000u | (static_cast<uint32_t>(em & 0x3ffu) << 13);   // inf, NaN
    } else if (em >= 0x0400u) {
        b = sign | ((em << 13) + (112u << 23));                                 // normal
    } else {
        const float f = static_cast<float>(em) * 0x1p-24f;                      // denormal or zero: exact
        std::memcpy(&b, &f, 4);
        b |= sign;
    }
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// The halving tree of 8f over 256 lane sums.
float tree256(float *s) {
    for (int h = 128; h > 0; h >>= 1)
        for (int j = 0; j < h; ++j) s[j] = s[j] + s[j + h];
    return s[0];
}

// One row of V widened logits -> token, {m, Z}.
void token_row_host(const float *x, size_t V, int32_t *token, float *stats) {
    const float inf = std::numeric_limits<float>::infinity(), qnan = dllm::token::exp_le0(std::nanf(""));
    // 1. the closed form of the fold
    ptrdiff_t n = -1;
    for (size_t i = 0; i < V; ++i)
        if (x[i] != x[i]) n = static_cast<ptrdiff_t>(i);
    size_t tok = V - 1;
    if (static_cast<size_t>(n + 1) < V) {
        tok = static_cast<size_t>(n + 1);
        for (size_t i = tok + 1; i < V; ++i)
            if (!(x[tok] > x[i])) tok = i;
    }
    *token = static_cast<int32_t>(tok);
    if (n >= 0) {
        stats[0] = stats[1] = qnan;
        return;
    }
    // 3. chunk partials (no NaN from here on)
    const size_t C = (V + kTokChunk - 1) / kTokChunk;
    std::vector<float> mc(C), Zc(C);
    float m = -inf;
    for (size_t c = 0; c < C; ++c) {
        const size_t lo = c * kTokChunk, hi = std::min(V, lo + kTokChunk);
        float mm = -inf;
        for (size_t i = lo; i < hi; ++i) mm = x[i] > mm ? x[i] : mm;
        mm = mm + 0.0f;
        mc[c] = mm;
        m = mm > m ? mm : m;
        if (mm == -inf || mm == inf) {
            Zc[c] = mm == inf ? qnan : 0.0f;
            continue;
        }
        float lane[256];
        for (float &l : lane) l = 0.0f;
        for (size_t i = lo; i < hi; ++i) {   // ascending i: each lane meets its groups in increasing g, components 0..3
            float &l = lane[((i - lo) / 4) % 256];
            l = l + dllm::token::exp_le0(x[i] - mm);
        }
        Zc[c] = tree256(lane);
    }
    // 4. the row
    stats[0] = m;
    if (m == -inf || m == inf) {
        stats[1] = m == inf ? qnan : 0.0f;
        return;
    }
    float lane[256];
    for (float &l : lane) l = 0.0f;
    for (size_t c = 0; c < C; ++c) lane[c % 256] = lane[c % 256] + (mc[c] == -inf ? 0.0f : Zc[c] * dllm::token::exp_le0(mc[c] - m));
    stats[1] = tree256(lane);
}

// ---- the token sampling rule in plain C++ (include/dllm_quant.h 8j; csrc/token.hip is the device form) ----

// Rule 5: the first j with t < F_j, F the sequential fold of a[0 .. n) from +0, t = RN(v F_{n-1}); -1 if none.
ptrdiff_t pick_host(const float *a, size_t n, float v) {
    float S = 0.0f;
    for (size_t j = 0; j < n; ++j) S = S + a[j];
    const float t = v * S;
    float F = 0.0f;
    for (size_t j = 0; j < n; ++j) {
        F = F + a[j];
        if (t < F) return static_cast<ptrdiff_t>(j);
    }
    return -1;
}

// The masks of 8k in fixed point; off = {1 << 32 (top_p == 1), 0}.
struct NucleusParams {
    bool p_on;
    uint64_t pfix, mfix;
};

// 8k.2 - 8k.4 on a row without a NaN: the larger of tau_p and tau_m (-inf when both masks are off).
// tau_k is the top-k threshold (-inf when off).  Literally the rule: the weights, then a walk down the
// sorted row for top-p and a minimum over the qualifying set for min-p.
float nucleus_tau_host(const std::vector<float> &y, size_t V, float tau_k, const NucleusParams &np) {
    const float inf = std::numeric_limits<float>::infinity();
    float m = -inf;
    for (size_t i = 0; i < V; ++i) m = y[i] > m ? y[i] : m;
    m = m + 0.0f;
    if (m == -inf || m == inf) return -inf;             // degenerate: the caller reports NaN
    std::vector<std::pair<float, uint64_t>> e(V);
    uint64_t T = 0;
    for (size_t i = 0; i < V; ++i) {
        const uint64_t W = y[i] >= tau_k ? dllm::token::nucleus_weight(dllm::token::exp_le0(y[i] - m)) : 0;
        e[i] = {y[i], W};
        T += W;
    }
    float tau = -inf;
    if (np.p_on) {
        std::sort(e.begin(), e.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
        uint64_t A = 0;
        for (size_t i = 0; i < V;) {                    // one distinct value (-0 == +0) per trip
            size_t j = i;
            for (; j < V && e[j].first == e[i].first; ++j) A += e[j].second;
            if ((static_cast<unsigned __int128>(A) << 32) >= static_cast<unsigned __int128>(np.pfix) * T) {
                tau = e[i].first;
                break;
            }
            i = j;
        }
    }
    if (np.mfix) {
        float tm = inf;
        for (size_t i = 0; i < V; ++i)
            if (e[i].second >= np.mfix && e[i].first < tm) tm = e[i].first;
        tau = tm > tau ? tm : tau;
    }
    return tau;
}

// One row of V widened logits -> token, {m, Z, p_token} and, with tau_out, the threshold of 8k.5.
// y is scratch of V floats.
void token_sample_row_host(const float *x, size_t V, float r, size_t top_k, const float *u, std::vector<float> &y,
                           int32_t *token, float *stats, const NucleusParams &np = {false, 0, 0},
                           float *tau_out = nullptr) {
    const float inf = std::numeric_limits<float>::infinity(), qnan = dllm::token::exp_le0(std::nanf(""));
    *token = -1;
    stats[0] = stats[1] = stats[2] = qnan;
    if (tau_out) *tau_out = qnan;
    // 1. temperature
    bool nan = false;
    for (size_t i = 0; i < V; ++i) {
        y[i] = x[i] * r;
        nan |= y[i] != y[i];
    }
    if (nan) return;
    // 2. top-k: tau = the k-th largest value; then 8k's thresholds; everything below becomes -inf
    float tau = -inf;
    if (top_k > 0 && top_k < V) {
        std::vector<float> v(y.begin(), y.end());
        std::nth_element(v.begin(), v.begin() + static_cast<ptrdiff_t>(top_k - 1), v.end(), std::greater<float>());
        tau = v[top_k - 1];
    }
    if (np.p_on || np.mfix) {
        const float t = nucleus_tau_host(y, V, tau, np);
        tau = t > tau ? t : tau;
    }
    tau = tau + 0.0f;                                    // a zero threshold is +0
    if (tau != -inf)
        for (size_t i = 0; i < V; ++i)
            if (!(y[i] >= tau)) y[i] = -inf;
    // 3. chunk partials and the row, as 8h.3 and 8h.4 (the lane sums are kept: level 2 picks among them)
    const size_t C = (V + kTokChunk - 1) / kTokChunk;
    std::vector<float> mc(C), w(C), lanes(C * 256, 0.0f);
    float m = -inf;
    for (size_t c = 0; c < C; ++c) {
        const size_t lo = c * kTokChunk, hi = std::min(V, lo + kTokChunk);
        float mm = -inf;
        for (size_t i = lo; i < hi; ++i) mm = y[i] > mm ? y[i] : mm;
        mm = mm + 0.0f;
        mc[c] = mm;
        m = mm > m ? mm : m;
        if (mm == -inf || mm == inf) continue;
        float *lane = &lanes[c * 256];
        for (size_t i = lo; i < hi; ++i) {
            float &l = lane[((i - lo) / 4) % 256];
            l = l + dllm::token::exp_le0(y[i] - mm);
        }
    }
    if (m == -inf || m == inf) return;
    if (tau_out) *tau_out = tau;
    float lane[256], tree[256];
    for (float &l : lane) l = 0.0f;
    for (size_t c = 0; c < C; ++c) {
        if (mc[c] == -inf) {
            w[c] = 0.0f;
        } else {
            std::memcpy(tree, &lanes[c * 256], sizeof(tree));
            w[c] = tree256(tree) * dllm::token::exp_le0(mc[c] - m);
        }
        lane[c % 256] = lane[c % 256] + w[c];
    }
    const float Z = tree256(lane);
    stats[0] = m;
    stats[1] = Z;
    // 5, 6. chunk, lane, element
    const ptrdiff_t c = pick_host(w.data(), C, u[0]);
    if (c < 0) return;
    const ptrdiff_t j = pick_host(&lanes[static_cast<size_t>(c) * 256], 256, u[1]);
    if (j < 0) return;
    float e[64];
    size_t at[64];
    for (size_t q = 0; q < 64; ++q) {
        at[q] = kTokChunk * static_cast<size_t>(c) + 4 * (256 * (q / 4) + static_cast<size_t>(j)) + q % 4;
        e[q] = at[q] < V ? dllm::token::exp_le0(y[at[q]] - mc[static_cast<size_t>(c)]) : 0.0f;
    }
    const ptrdiff_t q = pick_host(e, 64, u[2]);
    if (q < 0) return;
    // 7. the token and its probability
    *token = static_cast<int32_t>(at[q]);
    stats[2] = dllm::token::exp_le0(y[at[q]] - m) / Z;
}
}  // namespace

extern "C" {

int dllm_search_table_host(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                           float *table) {
    if (int rc = dllm::search::check_store_shape(rows, dim)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!codes || !scales || !zps || !table) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    for (size_t r = 0; r < rows; ++r) {
        uint32_t c1 = 0, c2 = 0;
        for (size_t d = 0; d < dim; ++d) {
            const uint32_t c = codes[r * dim + d];
            c1 += c;
            c2 += c * c;
        }
        const double s = scales[r], z = zps[r];
        const double nb2 = ((s * s) * static_cast<double>(c2) + ((2.0 * s) * z) * static_cast<double>(c1)) +
                           (z * z) * static_cast<double>(dim);
        const float w = nb2 > 0.0 ? static_cast<float>(1.0 / std::sqrt(nb2)) : 0.0f;
        table[2 * r] = scales[r] * w;
        table[2 * r + 1] = zps[r] * w;
    }
    return DLLM_OK;
}

int dllm_search_vectors_host(const float *Q, size_t nq, const uint8_t *codes, const float *table, size_t rows,
                             size_t dim, size_t k, int32_t *idx, float *scores) {
    if (int rc = dllm::search::check_k(k)) return rc;
    if (int rc = dllm::search::check_store_shape(rows, dim)) return rc;
    if (nq == 0) return DLLM_OK;
    if (!Q || !idx || !scores || (rows && (!codes || !table)))
        return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    std::vector<float> sc(rows);
    std::vector<uint64_t> keys(rows);
    const size_t top = std::min(k, rows);
    for (size_t j = 0; j < nq; ++j) {
        const float *q = Q + j * dim;
        const float qs = strand_sum(q, nullptr, false, dim), qn = strand_sum(q, nullptr, true, dim);
        const float wq = qn > 0.0f ? 1.0f / std::sqrt(qn) : 0.0f;
        for (size_t r = 0; r < rows; ++r) {
            const float A = strand_sum(q, codes + r * dim, false, dim);
            const float vq = table[2 * r + 1] * qs;
            sc[r] = std::fmaf(table[2 * r], A, vq) * wq;
            keys[r] = search_key(sc[r], static_cast<uint32_t>(r));
        }
        std::partial_sort(keys.begin(), keys.begin() + top, keys.end(), std::greater<uint64_t>());
        for (size_t i = 0; i < k; ++i) {
            const uint32_t id = i < top ? ~static_cast<uint32_t>(keys[i]) : 0u;
            idx[j * k + i] = i < top ? static_cast<int32_t>(id) : -1;
            scores[j * k + i] = i < top ? sc[id] : -std::numeric_limits<float>::infinity();
        }
    }
    return DLLM_OK;
}

// ---- section 8l on host slices: the rule of neighbor_rule.hpp row by row, ranked with a sort ----

size_t dllm_neighbor_table_bytes(size_t rows) { return rows * sizeof(dllm::neighbor::Entry); }

int dllm_neighbor_table_host(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                             void *table) {
    if (int rc = dllm::search::check_store_shape(rows, dim)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!codes || !scales || !zps || !table) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (int rc = dllm::neighbor::check_table_aligned(table)) return rc;
    dllm::neighbor::Entry *out = static_cast<dllm::neighbor::Entry *>(table);
    for (size_t r = 0; r < rows; ++r) {
        uint32_t c1 = 0, c2 = 0;
        for (size_t d = 0; d < dim; ++d) {
            const uint32_t c = codes[r * dim + d];
            c1 += c;
            c2 += c * c;
        }
        out[r] = dllm::neighbor::make_entry(scales[r], zps[r], c1, c2, static_cast<uint32_t>(dim));
    }
    return DLLM_OK;
}

int dllm_neighbor_rows_host(const uint8_t *qcodes, const void *qtable, size_t nq, const uint8_t *codes,
                            const void *table, size_t rows, size_t dim, size_t k, float threshold, int64_t self_base,
                            int32_t *idx, float *scores) {
    namespace nb = dllm::neighbor;
    if (int rc = nb::check_rows_args(nq, rows, dim, k, threshold, self_base)) return rc;
    if (nq == 0) return DLLM_OK;
    if (int rc = nb::check_rows_buffers(qcodes, qtable, codes, table, rows, idx, scores)) return rc;
    const nb::Entry *qt = static_cast<const nb::Entry *>(qtable), *tt = static_cast<const nb::Entry *>(table);
    std::vector<float> sc(rows);
    std::vector<uint64_t> keys;
    keys.reserve(rows);
    for (size_t j = 0; j < nq; ++j) {
        keys.clear();
        for (size_t t = 0; t < rows; ++t) {
            uint32_t D = 0;                                 // < 2^32: dim <= 65535
            for (size_t d = 0; d < dim; ++d) D += static_cast<uint32_t>(qcodes[j * dim + d]) * codes[t * dim + d];
            sc[t] = nb::score(qt[j].a, qt[j].b, qt[j].c1, tt[t].a, tt[t].b, tt[t].c1, D, static_cast<uint32_t>(dim));
            if (!nb::dropped(sc[t], threshold, self_base, j, t)) keys.push_back(search_key(sc[t], static_cast<uint32_t>(t)));
        }
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
        for (size_t i = 0; i < k; ++i) {
            const bool has = i < keys.size();
            const uint32_t id = has ? ~static_cast<uint32_t>(keys[i]) : 0u;
            idx[j * k + i] = has ? static_cast<int32_t>(id) : -1;
            scores[j * k + i] = has ? sc[id] : -std::numeric_limits<float>::infinity();
        }
    }
    return DLLM_OK;
}

int dllm_token_readout_host(const void *logits, int dtype, size_t M, size_t V, size_t ld, int32_t *tokens,
                            float *stats, float *probs) {
    if (int rc = dllm::token::check_logits(V, ld, dtype, false)) return rc;
    if (M == 0) return DLLM_OK;
    if (!logits || !tokens || !stats) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    const float ninf = -std::numeric_limits<float>::infinity(), qnan = dllm::token::exp_le0(std::nanf(""));
    std::vector<float> x(V);
    for (size_t b = 0; b < M; ++b) {
        for (size_t i = 0; i < V; ++i)
            x[i] = dtype == DLLM_F16 ? half_bits_to_float(static_cast<const uint16_t *>(logits)[b * ld + i])
                                     : static_cast<const float *>(logits)[b * ld + i];
        token_row_host(x.data(), V, tokens + b, stats + 2 * b);
        if (!probs) continue;
        const float m = stats[2 * b], Z = stats[2 * b + 1];
        const bool undefined = Z != Z || m == ninf;
        for (size_t i = 0; i < V; ++i) probs[b * V + i] = undefined ? qnan : dllm::token::exp_le0(x[i] - m) / Z;
    }
    return DLLM_OK;
}

int dllm_token_sample_host(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature,
                           size_t top_k, const float *u, uint64_t seed, uint64_t offset, int32_t *tokens,
                           float *stats) {
    float r;
    if (int rc = dllm::token::check_sample_args(V, ld, dtype, temperature, r)) return rc;
    if (M == 0) return DLLM_OK;
    if (!logits || !tokens || !stats) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    std::vector<float> x(V), y(V);
    for (size_t b = 0; b < M; ++b) {
        for (size_t i = 0; i < V; ++i)
            x[i] = dtype == DLLM_F16 ? half_bits_to_float(static_cast<const uint16_t *>(logits)[b * ld + i])
                                     : static_cast<const float *>(logits)[b * ld + i];
        float ub[3];
        if (u)
            std::memcpy(ub, u + 3 * b, sizeof(ub));
        else
            dllm::token::sample_uniforms(seed, offset + b, ub);
        token_sample_row_host(x.data(), V, r, top_k, ub, y, tokens + b, stats + 3 * b);
    }
    return DLLM_OK;
}

int dllm_token_sample_ex_host(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature,
                              size_t top_k, float top_p, float min_p, const float *u, uint64_t seed, uint64_t offset,
                              int32_t *tokens, float *stats) {
    float r;
    if (int rc = dllm::token::check_sample_ex_args(V, ld, dtype, temperature, top_p, min_p, r)) return rc;
    if (M == 0) return DLLM_OK;
    if (!logits || !tokens || !stats) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    const NucleusParams np{top_p != 1.0f, dllm::token::nucleus_pfix(top_p), dllm::token::nucleus_mfix(min_p)};
    std::vector<float> x(V), y(V);
    for (size_t b = 0; b < M; ++b) {
        for (size_t i = 0; i < V; ++i)
            x[i] = dtype == DLLM_F16 ? half_bits_to_float(static_cast<const uint16_t *>(logits)[b * ld + i])
                                     : static_cast<const float *>(logits)[b * ld + i];
        float ub[3], st[3];
        if (u)
            std::memcpy(ub, u + 3 * b, sizeof(ub));
        else
            dllm::token::sample_uniforms(seed, offset + b, ub);
        token_sample_row_host(x.data(), V, r, top_k, ub, y, tokens + b, st, np, stats + 4 * b + 3);
        std::memcpy(stats + 4 * b, st, sizeof(st));
    }
    return DLLM_OK;
}

// ---- the dedup rules in plain C++ (include/dllm_quant.h 8i; csrc/dedup.hip is the device form) ----

int dllm_hash_rows_host(const uint8_t *codes, size_t rows, size_t dim, size_t ld, uint64_t *hashes) {
    if (int rc = dllm::dedup::check_hash_args(rows, dim, ld)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!codes || !hashes) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    for (size_t r = 0; r < rows; ++r) {   // compute_hash, io-dedup/src/lib.rs:161-166
        uint64_t acc = 0;
        for (size_t i = 0; i < dim; ++i) acc = acc * 31u + codes[r * ld + i];
        hashes[r] = acc;
    }
    return DLLM_OK;
}

size_t dllm_dedup_table_bytes(size_t slots) {
    using namespace dllm::dedup;
    return slots_ok(slots) ? table_words(slots) * sizeof(uint64_t) : 0;
}

int dllm_dedup_table_init_host(void *table, size_t slots) {
    using namespace dllm::dedup;
    if (int rc = check_slots(slots)) return rc;
    if (!table) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    uint64_t *t = static_cast<uint64_t *>(table);
    std::fill(t, t + table_words(slots), ~uint64_t(0));
    t[kFlagWord] = t[kCountWord] = t[3] = 0;
    return DLLM_OK;
}

int dllm_dedup_rows_host(const uint64_t *hashes, size_t rows, uint64_t base, void *table, size_t slots, uint8_t *keep,
                         uint64_t *first, int32_t *kept_rows, uint32_t *n_kept) {
    using namespace dllm::dedup;
    if (int rc = check_filter_args(rows, base, table, slots)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!hashes || !keep || !first || !kept_rows || !n_kept) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    std::unordered_map<uint64_t, uint64_t> seen;   // the one-shot form's set: hash -> first sequence number
    uint64_t *t = static_cast<uint64_t *>(table);
    uint32_t n = 0;
    for (size_t r = 0; r < rows; ++r) {             // deduplicate, io-dedup/src/lib.rs:145-159
        const uint64_t h = hashes[r], seq = base + r;
        uint64_t *val = nullptr;                    // where this hash's first sequence number lives
        bool fresh = false;
        if (!t) {
            auto ins = seen.emplace(h, seq);
            val = &ins.first->second, fresh = ins.second;
        } else if (h == kEmptyKey) {
            val = t + kSideWord, fresh = *val == kNoSeq;
        } else {
            uint64_t *keys = t + kHeaderWords, *vals = keys + slots;
            size_t s = first_slot(h, slots - 1);
            for (size_t probe = 0; probe < slots && !val; ++probe) {
                if (keys[s] == kEmptyKey) keys[s] = h, fresh = true;
                if (keys[s] == h) val = vals + s;
                s = (s + 1) & (slots - 1);
            }
        }
        if (!val) {                                 // no slot left: only a dishonest base gets here
            t[kFlagWord] = 1;
            keep[r] = 0, first[r] = kNoSeq;
            continue;
        }
        if (fresh) {
            *val = seq;
            if (t) ++t[kCountWord];
        }
        keep[r] = fresh ? 1 : 0;
        first[r] = *val;
        if (fresh) kept_rows[n++] = static_cast<int32_t>(r);
    }
    *n_kept = n;
    for (size_t i = n; i < rows; ++i) kept_rows[i] = -1;
    return DLLM_OK;
}

int dllm_gather_rows_host(const uint8_t *codes, size_t dim, size_t ld, const int32_t *kept_rows, const uint32_t *n_kept,
                          uint8_t *out, size_t out_ld) {
    if (int rc = dllm::dedup::check_gather_args(dim, ld, out_ld)) return rc;
    if (!codes || !kept_rows || !n_kept || !out) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    for (size_t i = 0; i < *n_kept; ++i)            // merge_requests' concat, io-dedup/src/lib.rs:181-212
        if (kept_rows[i] >= 0) std::memcpy(out + i * out_ld, codes + static_cast<size_t>(kept_rows[i]) * ld, dim);
    return DLLM_OK;
}

}  // extern "C"
