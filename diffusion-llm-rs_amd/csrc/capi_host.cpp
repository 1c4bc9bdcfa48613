// capi_host.cpp -- host-slice entry points (*_host): the literal shapes of the reference's Rust
// signatures (&[f32] in, Vec<u8> / Vec<f32> out).  Each call stages through device memory on its
// own stream, runs the same HIP kernels as the device entry points, and synchronises.
#include <hip/hip_runtime.h>

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
#include "neighbor_rule.hpp"
#include "token_exp.hpp"
#include "token_nucleus_rule.hpp"
#include "token_sample_rule.hpp"

namespace dllm {
int fail(int code, const std::string &msg);
}

namespace {

struct Staging {
    std::vector<void *> bufs;
    hipStream_t st = nullptr;
    int err = DLLM_OK;
    Staging() {
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
            st = nullptr;
            err = dllm::fail(DLLM_ERR_HIP, "hipStreamCreate failed (no device?)");
        }
    }
    ~Staging() {
        for (void *p : bufs) (void)hipFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
    template <typename T>
    T *alloc(size_t count) {
        void *p = nullptr;
        if (hipMalloc(&p, count * sizeof(T) + 16) != hipSuccess) {
            err = dllm::fail(DLLM_ERR_HIP, "hipMalloc failed");
            return nullptr;
        }
        bufs.push_back(p);
        return static_cast<T *>(p);
    }
    template <typename T>
    T *upload(const T *h, size_t count) {
        T *d = alloc<T>(count);
        if (d && count && hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess)
            err = dllm::fail(DLLM_ERR_HIP, "hipMemcpy H2D failed");
        return d;
    }
    template <typename T>
    int download(T *h, const T *d, size_t count) {
        if (count && hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess)
            return dllm::fail(DLLM_ERR_HIP, "hipMemcpy D2H failed");
        return DLLM_OK;
    }
    int sync() {
        if (hipStreamSynchronize(st) != hipSuccess) return dllm::fail(DLLM_ERR_HIP, "hipStreamSynchronize failed");
        return DLLM_OK;
    }
};

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

uint64_t search_key(float s, uint32_t idx) {
    uint32_t b;
    std::memcpy(&b, &s, 4);
    uint32_t ord;
    if (s != s) {
        ord = 0u;
    } else {
        if (b == 0x80000000u) b = 0u;
        ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return (static_cast<uint64_t>(ord) << 32) | static_cast<uint32_t>(~idx);
}

int search_shape_ok(size_t rows, size_t dim) {
    if (dim == 0 || dim > 65535) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "dim must be between 1 and 65535");
    if (rows >= (size_t(1) << 31))
        return dllm::fail(DLLM_ERR_SHAPE_MISMATCH, "rows must be below 2^31 (the index is an int32)");
    return DLLM_OK;
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

constexpr size_t kTokenChunk = 16384;

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
    const size_t C = (V + kTokenChunk - 1) / kTokenChunk;
    std::vector<float> mc(C), Zc(C);
    float m = -inf;
    for (size_t c = 0; c < C; ++c) {
        const size_t lo = c * kTokenChunk, hi = std::min(V, lo + kTokenChunk);
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
    const size_t C = (V + kTokenChunk - 1) / kTokenChunk;
    std::vector<float> mc(C), w(C), lanes(C * 256, 0.0f);
    float m = -inf;
    for (size_t c = 0; c < C; ++c) {
        const size_t lo = c * kTokenChunk, hi = std::min(V, lo + kTokenChunk);
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
        at[q] = kTokenChunk * static_cast<size_t>(c) + 4 * (256 * (q / 4) + static_cast<size_t>(j)) + q % 4;
        e[q] = at[q] < V ? dllm::token::exp_le0(y[at[q]] - mc[static_cast<size_t>(c)]) : 0.0f;
    }
    const ptrdiff_t q = pick_host(e, 64, u[2]);
    if (q < 0) return;
    // 7. the token and its probability
    *token = static_cast<int32_t>(at[q]);
    stats[2] = dllm::token::exp_le0(y[at[q]] - m) / Z;
}

#define STAGE_OK(s) \
    do {            \
        if ((s).err) return (s).err; \
    } while (0)

}  // namespace

extern "C" {

int dllm_quantize_tensor_host(const float *x, size_t n, uint8_t bits, uint8_t *codes, float *scale, float *zp) {
    if (bits < 1 || bits > 8) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "Bits must be between 1 and 8");
    Staging s;
    STAGE_OK(s);
    const float *dx = s.upload(x, n);
    uint8_t *dq = s.alloc<uint8_t>(n);
    float *dp = s.alloc<float>(2);
    const size_t wsb = dllm_quantize_tensor_workspace(n);
    void *ws = s.alloc<uint8_t>(wsb);
    STAGE_OK(s);
    int rc = dllm_quantize_tensor(dx, n, bits, 0, dq, dp, ws, wsb, s.st);
    if (rc) return rc;
    float p[2];
    if ((rc = s.download(codes, dq, n)) || (rc = s.download(p, dp, 2)) || (rc = s.sync())) return rc;
    *scale = p[0];
    *zp = p[1];
    return DLLM_OK;
}

int dllm_dequantize_tensor_host(const uint8_t *codes, size_t n, float scale, float zp, float *out) {
    Staging s;
    STAGE_OK(s);
    const uint8_t *dq = s.upload(codes, n);
    float *dy = s.alloc<float>(n);
    STAGE_OK(s);
    int rc = dllm_dequantize_tensor_scalar(dq, n, 8, 0, scale, zp, dy, DLLM_F32, s.st);
    if (rc || (rc = s.download(out, dy, n)) || (rc = s.sync())) return rc;
    return DLLM_OK;
}

int dllm_default_quantize_host(const float *x, size_t n, int qtype, float scale, int32_t zero_point, uint8_t *out) {
    Staging s;
    STAGE_OK(s);
    const float *dx = s.upload(x, n);
    uint8_t *dq = s.alloc<uint8_t>(n);
    STAGE_OK(s);
    int rc = dllm_default_quantize(dx, n, qtype, scale, zero_point, dq, s.st);
    if (rc || (rc = s.download(out, dq, n)) || (rc = s.sync())) return rc;
    return DLLM_OK;
}

int dllm_default_dequantize_host(const uint8_t *q, size_t n, float scale, int32_t zero_point, float *out) {
    Staging s;
    STAGE_OK(s);
    const uint8_t *dq = s.upload(q, n);
    float *dy = s.alloc<float>(n);
    STAGE_OK(s);
    int rc = dllm_default_dequantize(dq, n, scale, zero_point, dy, s.st);
    if (rc || (rc = s.download(out, dy, n)) || (rc = s.sync())) return rc;
    return DLLM_OK;
}

int dllm_bit_quantize_host(const float *x, size_t n, uint32_t bits, float scale, float zero_point, uint8_t *out) {
    if (bits > 30) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "(1 << bits) - 1 overflows i32");
    Staging s;
    STAGE_OK(s);
    const float *dx = s.upload(x, n);
    uint8_t *dq = s.alloc<uint8_t>(n);
    STAGE_OK(s);
    int rc = dllm_bit_quantize(dx, n, bits, scale, zero_point, dq, s.st);
    if (rc || (rc = s.download(out, dq, n)) || (rc = s.sync())) return rc;
    return DLLM_OK;
}

int dllm_bit_dequantize_host(const uint8_t *q, size_t n, float scale, float zero_point, float *out) {
    Staging s;
    STAGE_OK(s);
    const uint8_t *dq = s.upload(q, n);
    float *dy = s.alloc<float>(n);
    STAGE_OK(s);
    int rc = dllm_bit_dequantize(dq, n, scale, zero_point, dy, DLLM_F32, s.st);
    if (rc || (rc = s.download(out, dy, n)) || (rc = s.sync())) return rc;
    return DLLM_OK;
}

int dllm_compress_vector_host(const float *x, size_t n, uint8_t bits, uint8_t *out, float *scale, float *zp) {
    Staging s;
    STAGE_OK(s);
    const float *dx = s.upload(x, n);
    uint8_t *dq = s.alloc<uint8_t>(n);
    float *dsc = s.alloc<float>(1);
    float *dzp = s.alloc<float>(1);
    STAGE_OK(s);
    int rc = dllm_compress_vectors(dx, 1, n, bits, dq, dsc, dzp, s.st);
    if (rc || (rc = s.download(out, dq, n)) || (rc = s.download(scale, dsc, 1)) || (rc = s.download(zp, dzp, 1)) ||
        (rc = s.sync()))
        return rc;
    return DLLM_OK;
}

int dllm_linear_create_host(const float *W, const float *bias, size_t K, size_t N, uint8_t bits, size_t group,
                            dllm_linear_t *out) {
    Staging s;
    STAGE_OK(s);
    const float *dW = s.upload(W, K * N);
    const float *db = bias ? s.upload(bias, N) : nullptr;
    STAGE_OK(s);
    int rc = dllm_linear_create(dW, db, K, N, bits, group, out, s.st);
    if (rc) return rc;
    return s.sync();
}

int dllm_linear_forward_host(dllm_linear_t h, const float *X, size_t M, float *Y) {
    size_t K = 0, N = 0;
    int rc = dllm_linear_info(h, &K, &N, nullptr, nullptr);
    if (rc) return rc;
    Staging s;
    STAGE_OK(s);
    const float *dX = s.upload(X, M * K);
    float *dY = s.alloc<float>(M * N);
    STAGE_OK(s);
    if ((rc = dllm_linear_forward(h, dX, M, DLLM_F32, dY, DLLM_F32, s.st))) return rc;
    if ((rc = s.download(Y, dY, M * N)) || (rc = s.sync())) return rc;
    return DLLM_OK;
}

int dllm_p_losses_host(dllm_linear_t h, const float *betas, size_t T, const float *x_start, const size_t *t,
                       const float *noise, uint64_t seed, uint64_t offset, size_t B, size_t D, float *loss) {
    size_t K = 0, N = 0;
    int rc = dllm_linear_info(h, &K, &N, nullptr, nullptr);
    if (rc) return rc;
    if (D != K || D != N)
        return dllm::fail(DLLM_ERR_SHAPE_MISMATCH, "Noise shape must match input shape: D must equal the model's K and N");
    if (B && (!x_start || !loss)) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    std::vector<float> coef(2 * B);
    if ((rc = dllm_p_losses_coeffs(betas, T, t, B, coef.data()))) return rc;
    if (B == 0) return DLLM_OK;
    Staging s;
    STAGE_OK(s);
    const float *dx = s.upload(x_start, B * D);
    const float *dn = noise ? s.upload(noise, B * D) : nullptr;
    const float *dc = s.upload(coef.data(), 2 * B);
    float *dnoisy = s.alloc<float>(B * D);
    float *deps = s.alloc<float>(B * D);
    float *dloss = s.alloc<float>(B);
    const size_t wsb = dllm_noise_mse_workspace(B, D);
    void *ws = s.alloc<uint8_t>(wsb);
    STAGE_OK(s);
    if ((rc = dllm_add_noise(dx, dn, dc, B, D, seed, offset, dnoisy, nullptr, s.st))) return rc;
    if ((rc = dllm_linear_forward(h, dnoisy, B, DLLM_F32, deps, DLLM_F32, s.st))) return rc;
    if ((rc = dllm_noise_mse(deps, DLLM_F32, dn, B, D, seed, offset, dloss, ws, wsb, s.st))) return rc;
    if ((rc = s.download(loss, dloss, B)) || (rc = s.sync())) return rc;
    return DLLM_OK;
}

int dllm_search_table_host(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                           float *table) {
    if (int rc = search_shape_ok(rows, dim)) return rc;
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
    if (k == 0 || k > 256) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "k must be between 1 and 256");
    if (int rc = search_shape_ok(rows, dim)) return rc;
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

int dllm_neighbor_table_host(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                             void *table) {
    if (int rc = search_shape_ok(rows, dim)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!codes || !scales || !zps || !table) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(table) % 8) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "table must be 8-byte aligned");
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
    if (k == 0 || k > nb::kMaxK) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "k must be between 1 and 256");
    if (int rc = search_shape_ok(rows, dim)) return rc;
    if (threshold != threshold) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "threshold must not be NaN");
    if (self_base < -1) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "self_base must be -1 or a row of the store");
    if (self_base >= 0 && (static_cast<uint64_t>(self_base) > rows || nq > rows - static_cast<uint64_t>(self_base)))
        return dllm::fail(DLLM_ERR_INVALID_PARAMS, "self_base + nq exceeds rows");
    if (nq == 0) return DLLM_OK;
    if (!qcodes || !qtable || !idx || !scores || (rows && (!codes || !table)))
        return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(qtable) % 8 || reinterpret_cast<uintptr_t>(table) % 8)
        return dllm::fail(DLLM_ERR_INVALID_PARAMS, "qtable and table must be 8-byte aligned");
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
    if (V == 0) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "V == 0: no token to read out of an empty vocabulary");
    if (ld < V) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least V");
    if (V >= (size_t(1) << 31))
        return dllm::fail(DLLM_ERR_SHAPE_MISMATCH, "V must be below 2^31 (the token is an int32)");
    if (dtype != DLLM_F32 && dtype != DLLM_F16)
        return dllm::fail(DLLM_ERR_UNSUPPORTED, "dtype must be DLLM_F32 or DLLM_F16");
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
    if (V == 0) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "V == 0: no token to sample from an empty vocabulary");
    if (ld < V) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least V");
    if (V >= (size_t(1) << 31))
        return dllm::fail(DLLM_ERR_SHAPE_MISMATCH, "V must be below 2^31 (the token is an int32)");
    if (dtype != DLLM_F32 && dtype != DLLM_F16)
        return dllm::fail(DLLM_ERR_UNSUPPORTED, "dtype must be DLLM_F32 or DLLM_F16");
    const float r = 1.0f / temperature;
    if (!(temperature > 0.0f) || !std::isfinite(temperature) || !std::isfinite(r))
        return dllm::fail(DLLM_ERR_INVALID_PARAMS, "temperature and 1 / temperature must be positive and finite");
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
    if (V == 0) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "V == 0: no token to sample from an empty vocabulary");
    if (ld < V) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least V");
    if (V >= (size_t(1) << 31))
        return dllm::fail(DLLM_ERR_SHAPE_MISMATCH, "V must be below 2^31 (the token is an int32)");
    if (dtype != DLLM_F32 && dtype != DLLM_F16)
        return dllm::fail(DLLM_ERR_UNSUPPORTED, "dtype must be DLLM_F32 or DLLM_F16");
    const float r = 1.0f / temperature;
    if (!(temperature > 0.0f) || !std::isfinite(temperature) || !std::isfinite(r))
        return dllm::fail(DLLM_ERR_INVALID_PARAMS, "temperature and 1 / temperature must be positive and finite");
    if (!(top_p > 0.0f) || top_p > 1.0f) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "top_p must be in (0, 1]");
    if (!(min_p >= 0.0f) || min_p > 1.0f) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "min_p must be in [0, 1]");
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
    if (dim == 0 || dim > dllm::dedup::kMaxDim) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "dim must be between 1 and 65535");
    if (ld < dim) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least dim");
    if (rows >= (size_t(1) << 31)) return dllm::fail(DLLM_ERR_SHAPE_MISMATCH, "rows must be below 2^31");
    if (rows == 0) return DLLM_OK;
    if (!codes || !hashes) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    for (size_t r = 0; r < rows; ++r) {   // compute_hash, io-dedup/src/lib.rs:161-166
        uint64_t acc = 0;
        for (size_t i = 0; i < dim; ++i) acc = acc * 31u + codes[r * ld + i];
        hashes[r] = acc;
    }
    return DLLM_OK;
}

int dllm_dedup_table_init_host(void *table, size_t slots) {
    using namespace dllm::dedup;
    if (!is_pow2(slots) || slots > (size_t(1) << 56)) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "slots must be a power of two");
    if (!table) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    uint64_t *t = static_cast<uint64_t *>(table);
    std::fill(t, t + table_words(slots), ~uint64_t(0));
    t[kFlagWord] = t[kCountWord] = t[3] = 0;
    return DLLM_OK;
}

int dllm_dedup_rows_host(const uint64_t *hashes, size_t rows, uint64_t base, void *table, size_t slots, uint8_t *keep,
                         uint64_t *first, int32_t *kept_rows, uint32_t *n_kept) {
    using namespace dllm::dedup;
    if (rows >= (size_t(1) << 31))
        return dllm::fail(DLLM_ERR_SHAPE_MISMATCH, "rows must be below 2^31 (a kept row's index is an int32)");
    if (base >= (uint64_t(1) << 62)) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "base must be below 2^62");
    if (table) {
        if (!is_pow2(slots) || slots > (size_t(1) << 56))
            return dllm::fail(DLLM_ERR_INVALID_PARAMS, "slots must be a power of two");
        if (reinterpret_cast<uintptr_t>(table) % 8) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "table must be 8-byte aligned");
        if (base + rows > slots / 2)
            return dllm::fail(DLLM_ERR_INVALID_PARAMS, "base + rows exceeds slots / 2: the seen-set is kept at most half full");
    }
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
    if (dim == 0 || dim > dllm::dedup::kMaxDim) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "dim must be between 1 and 65535");
    if (ld < dim) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least dim");
    if (out_ld < dim) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "out_ld must be at least dim");
    if (!codes || !kept_rows || !n_kept || !out) return dllm::fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    for (size_t i = 0; i < *n_kept; ++i)            // merge_requests' concat, io-dedup/src/lib.rs:181-212
        if (kept_rows[i] >= 0) std::memcpy(out + i * out_ld, codes + static_cast<size_t>(kept_rows[i]) * ld, dim);
    return DLLM_OK;
}

}  // extern "C"
