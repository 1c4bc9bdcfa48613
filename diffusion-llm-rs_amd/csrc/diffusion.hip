// diffusion.hip -- the elementwise ops either side of the denoiser in every timestep (SURVEY.md
// 8f rank 1): beta schedules and alpha-bar tables (host scalars, Rust f32 semantics), the
// p_sample posterior step and the add_noise forward step (HBM-bound kernels), and the seeded
// Gaussian noise they draw (Philox4x32-10 + a Box-Muller built only from correctly rounded
// + - * / sqrt, so it is reproducible bit for bit on any IEEE host), and the p_losses reduction
// (per-sample mean squared error of the predicted noise, in a summation order fixed by the header).
//
// Reference: diffuse-llm-rs/src/lib.rs create_beta_schedule :554-593, p_losses :595-653,
// add_noise :1100-1137, p_sample :1152-1215.
#include "common.hpp"
#include "diffusion_rng.hpp"

#include <cmath>
#include <vector>

namespace dllm {
namespace {

// ---- host scalars (per timestep / per sample) -------------------------------------------------

int alpha_tables(const float *betas, size_t T, int cumprod, std::vector<float> &alphas, std::vector<float> &abar) {
    alphas.resize(T);
    abar.resize(T);
    for (size_t i = 0; i < T; ++i) alphas[i] = 1.0f - betas[i];
    if (cumprod == DLLM_ABAR_INCLUSIVE) {          // p_losses scan, lib.rs:627-630
        float state = 1.0f;
        for (size_t i = 0; i < T; ++i) abar[i] = (state *= alphas[i]);
    } else if (cumprod == DLLM_ABAR_EXCLUSIVE) {   // add_noise / p_sample, lib.rs:1116-1119
        if (T) abar[0] = 1.0f;
        for (size_t i = 1; i < T; ++i) abar[i] = abar[i - 1] * alphas[i - 1];
    } else {
        return fail(DLLM_ERR_INVALID_PARAMS, "cumprod must be DLLM_ABAR_EXCLUSIVE or DLLM_ABAR_INCLUSIVE");
    }
    return DLLM_OK;
}

// ---- device ---------------------------------------------------------------------------------

// x_prev = (c1 x_t + c2 eps) + std * n over rows of D; n = noise[i] (given), the generated stream
// element offset + i (noise == nullptr), or 0 (add == 0).  Four consecutive elements per thread:
// one Philox block when offset % 4 == 0.
// out may be x or eps (dllm_p_sample: x_prev may alias x_t or eps): every element is read before it
// is written, by the one thread that owns it, so those three carry no __restrict__.
__global__ void __launch_bounds__(256) p_sample_kernel(const float *x, const float *eps,
                                                       const float *__restrict__ noise, const float *__restrict__ coef,
                                                       size_t n, size_t D, int add, uint64_t seed, uint64_t offset,
                                                       float *out) {
    const size_t nq = (n + 3) / 4;
    for (size_t q = blockIdx.x * static_cast<size_t>(256) + threadIdx.x; q < nq;
         q += static_cast<size_t>(gridDim.x) * 256) {
        const size_t i0 = q * 4;
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (add) {
            if (noise) {
                for (int l = 0; l < 4; ++l)
                    if (i0 + l < n) z[l] = noise[i0 + l];
            } else {
                rng::normal4(seed, (offset + i0) / 4, z);
            }
        }
        if (i0 + 4 <= n && (D % 4) == 0) {
            const float *c = coef + 3 * (i0 / D);
            const float c1 = c[0], c2 = c[1], sd = c[2];
            const float4 xv = *reinterpret_cast<const float4 *>(x + i0);
            const float4 ev = *reinterpret_cast<const float4 *>(eps + i0);
            float4 o;
            o.x = (c1 * xv.x + c2 * ev.x) + sd * z[0];
            o.y = (c1 * xv.y + c2 * ev.y) + sd * z[1];
            o.z = (c1 * xv.z + c2 * ev.z) + sd * z[2];
            o.w = (c1 * xv.w + c2 * ev.w) + sd * z[3];
            *reinterpret_cast<float4 *>(out + i0) = o;
        } else {
            for (int l = 0; l < 4; ++l) {
                const size_t i = i0 + l;
                if (i >= n) break;
                const float *c = coef + 3 * (i / D);
                out[i] = (c[0] * x[i] + c[1] * eps[i]) + c[2] * z[l];
            }
        }
    }
}

// noisy = x0 sqrt(abar) + n sqrt(1 - abar); n given or generated (then optionally written out).
// out may be x0 (dllm_add_noise: noisy may alias x0), so neither carries __restrict__.
__global__ void __launch_bounds__(256) add_noise_kernel(const float *x0, const float *__restrict__ noise,
                                                        const float *__restrict__ coef, size_t n, size_t D,
                                                        uint64_t seed, uint64_t offset, float *out,
                                                        float *__restrict__ noise_out) {
    const size_t nq = (n + 3) / 4;
    for (size_t q = blockIdx.x * static_cast<size_t>(256) + threadIdx.x; q < nq;
         q += static_cast<size_t>(gridDim.x) * 256) {
        const size_t i0 = q * 4;
        float z[4];
        if (noise) {
            for (int l = 0; l < 4; ++l) z[l] = i0 + l < n ? noise[i0 + l] : 0.f;
        } else {
            rng::normal4(seed, (offset + i0) / 4, z);
        }
        for (int l = 0; l < 4; ++l) {
            const size_t i = i0 + l;
            if (i >= n) break;
            const float *c = coef + 2 * (i / D);
            out[i] = x0[i] * c[0] + z[l] * c[1];
            if (noise_out) noise_out[i] = z[l];
        }
    }
}

__global__ void __launch_bounds__(256) randn_kernel(uint64_t seed, uint64_t offset, size_t n, float *__restrict__ out) {
    const size_t nq = (n + 3) / 4;
    for (size_t q = blockIdx.x * static_cast<size_t>(256) + threadIdx.x; q < nq;
         q += static_cast<size_t>(gridDim.x) * 256) {
        const size_t i0 = q * 4;
        float z[4];
        rng::normal4(seed, (offset + i0) / 4, z);   // the stream index wraps modulo 2^64, as in every consumer
        if (i0 + 4 <= n) {
            *reinterpret_cast<float4 *>(out + i0) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
            for (int l = 0; i0 + l < n; ++l) out[i0 + l] = z[l];
        }
    }
}

unsigned elem_grid(size_t n) { return grid_for((n + 3) / 4, 256, kCUs * 16); }

// ---- p_losses: per-sample mean of (noise - pred)^2 in the pinned order of dllm_noise_mse ---------

constexpr int kMseLanes = 256;                        // lanes of a chunk = threads of a block
constexpr int kMseTrips = 16;                         // groups of four per lane and chunk
constexpr size_t kMseChunk = 4 * kMseLanes * kMseTrips;   // 16384 elements

inline size_t mse_chunks(size_t n) { return (n + kMseChunk - 1) / kMseChunk; }

// The halving tree over the block's 256 lane sums: s[j] = s[j] + s[j + h] for j < h, h = 128 ... 1.
// Levels 128 and 64 cross waves (through LDS); 32 ... 1 stay in wave 0, where lane j < h takes
// exactly lane j + h's value of the level before.  The root is thread 0's return value.
__device__ __forceinline__ float mse_tree(float s, float *lds) {
    const int j = threadIdx.x;
    lds[j] = s;
    __syncthreads();
    if (j < 128) {
        s = s + lds[j + 128];
        lds[j] = s;
    }
    __syncthreads();
    if (j < 64) {
        s = s + lds[j + 64];
#pragma unroll
        for (int h = 32; h > 0; h >>= 1) s = s + __shfl_down(s, h, 64);
    }
    return s;
}

__device__ __forceinline__ float4 load_pred4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load_pred4(const __half *p) {
    const uint2 r = *reinterpret_cast<const uint2 *>(p);
    const __half2 lo = *reinterpret_cast<const __half2 *>(&r.x), hi = *reinterpret_cast<const __half2 *>(&r.y);
    return make_float4(__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi));
}

// s + (nz - p)^2 over the group's components 0..3, every op rounded once (-ffp-contract=off).
__device__ __forceinline__ float mse_add4(float s, const float4 nz, const float4 p) {
    float d = nz.x - p.x;
    s = s + d * d;
    d = nz.y - p.y;
    s = s + d * d;
    d = nz.z - p.z;
    s = s + d * d;
    d = nz.w - p.w;
    return s + d * d;
}

// Block (b, c) = blockIdx.x: chunk c of sample b -> partial[b C + c], or, for a one-chunk sample,
// whose total is that partial (the finish pass would add it to +0 only), loss[b] directly.  Groups
// past n are +0 terms of a sum that never goes below +0: leaving them out changes no bit.
// kStream: the noise is regenerated (noise == nullptr); an instantiation of its own, so that its
// register budget is not the explicit form's 32 loads in flight.
template <typename T, bool kStream>
__global__ void __launch_bounds__(kMseLanes) noise_mse_chunk_kernel(const T *__restrict__ pred,
                                                                    const float *__restrict__ noise, size_t n,
                                                                    size_t C, uint64_t seed, uint64_t offset,
                                                                    float *__restrict__ partial,
                                                                    float *__restrict__ loss) {
    __shared__ float lds[kMseLanes];
    const size_t b = blockIdx.x / C, c = blockIdx.x % C;
    const size_t base = b * n;                                        // first element of the sample
    const size_t i0 = c * kMseChunk + 4 * static_cast<size_t>(threadIdx.x);   // this lane's group of trip 0
    float s = 0.f;
    if constexpr (!kStream) {
        // HBM-bound: all 16 + 16 loads of the lane in flight before the first add
        float4 p[kMseTrips], z[kMseTrips];
#pragma unroll
        for (int k = 0; k < kMseTrips; ++k) {
            const size_t i = i0 + static_cast<size_t>(k) * (4 * kMseLanes);
            p[k] = i < n ? load_pred4(pred + base + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            z[k] = i < n ? *reinterpret_cast<const float4 *>(noise + base + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < kMseTrips; ++k) s = mse_add4(s, z[k], p[k]);
    } else if ((c + 1) * kMseChunk <= n) {
        // VALU-bound, a whole chunk (block-uniform): four trips per pass with no branch between them,
        // so four independent generator chains interleave and cover the pass's loads -- with 2-4
        // blocks per CU there are too few waves to hide one chain's latencies otherwise (all 16 at
        // once would take every register)
#pragma unroll 1
        for (int k0 = 0; k0 < kMseTrips; k0 += 4) {
            const size_t i = i0 + static_cast<size_t>(k0) * (4 * kMseLanes);
            float4 p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = load_pred4(pred + base + i + static_cast<size_t>(k) * (4 * kMseLanes));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float z[4];
                // the index wraps modulo 2^64 before the division, as in the ragged branch below
                rng::normal4(seed, (offset + base + i + static_cast<size_t>(k) * (4 * kMseLanes)) / 4, z);
                s = mse_add4(s, make_float4(z[0], z[1], z[2], z[3]), p[k]);
            }
        }
    } else {
        for (int k = 0; k < kMseTrips; ++k) {
            const size_t i = i0 + static_cast<size_t>(k) * (4 * kMseLanes);
            if (i < n) {
                const float4 p = load_pred4(pred + base + i);
                float z[4];
                rng::normal4(seed, (offset + base + i) / 4, z);
                s = mse_add4(s, make_float4(z[0], z[1], z[2], z[3]), p);
            }
        }
    }
    s = mse_tree(s, lds);
    if (threadIdx.x == 0) {
        if (C == 1)
            loss[b] = s / static_cast<float>(n);
        else
            partial[blockIdx.x] = s;
    }
}

template <typename T>
void launch_mse_chunks(const T *pred, const float *noise, size_t n, size_t C, uint64_t seed, uint64_t offset,
                       float *partial, float *loss, unsigned grid, hipStream_t st) {
    if (noise)
        noise_mse_chunk_kernel<T, false><<<grid, kMseLanes, 0, st>>>(pred, noise, n, C, seed, offset, partial, loss);
    else
        noise_mse_chunk_kernel<T, true><<<grid, kMseLanes, 0, st>>>(pred, noise, n, C, seed, offset, partial, loss);
}

// Block b: the sample's C partials to 256 lanes round-robin, the same tree, the division.
__global__ void __launch_bounds__(kMseLanes) noise_mse_finish_kernel(const float *__restrict__ partial, size_t n,
                                                                     size_t C, float *__restrict__ loss) {
    __shared__ float lds[kMseLanes];
    const float *P = partial + blockIdx.x * C;
    float s = 0.f;
    for (size_t c = threadIdx.x; c < C; c += kMseLanes) s = s + P[c];
    s = mse_tree(s, lds);
    if (threadIdx.x == 0) loss[blockIdx.x] = s / static_cast<float>(n);
}

}  // namespace
}  // namespace dllm

using namespace dllm;

extern "C" {

int dllm_beta_schedule(int kind, size_t T, float beta_start, float beta_end, float *betas) {
    if (T && !betas) return fail(DLLM_ERR_INVALID_PARAMS, "betas is NULL");
    const float PI = 3.14159274101257324f;   // std::f32::consts::PI (lib.rs:20)
    for (size_t t = 0; t < T; ++t) {
        float b;
        switch (kind) {
        case DLLM_BETA_LINEAR:       // lib.rs:559-564
            b = beta_start + (beta_end - beta_start) * static_cast<float>(t) / static_cast<float>(T - 1);
            break;
        case DLLM_BETA_QUADRATIC: {  // lib.rs:568-574
            const float tn = static_cast<float>(t) / static_cast<float>(T - 1);
            b = beta_start + (beta_end - beta_start) * tn * tn;
            break;
        }
        case DLLM_BETA_COSINE: {     // lib.rs:578-590
            const float s = 0.008f;
            const float tn = static_cast<float>(t) / static_cast<float>(T);
            float ft = std::cos((tn + s) / (1.0f + s) * PI / 2.0f);
            ft = ft * ft;
            float f0 = std::cos(s / (1.0f + s) * PI / 2.0f);
            f0 = f0 * f0;
            b = std::fmin(1.0f - ft / f0, 0.999f);
            break;
        }
        default:
            return fail(DLLM_ERR_INVALID_PARAMS, "unknown beta schedule kind");
        }
        betas[t] = b;
    }
    return DLLM_OK;
}

int dllm_alpha_bars(const float *betas, size_t T, int cumprod, float *alphas, float *alpha_bars) {
    if (T && (!betas || !alphas || !alpha_bars)) return fail(DLLM_ERR_INVALID_PARAMS, "NULL table");
    std::vector<float> a, ab;
    const int rc = alpha_tables(betas, T, cumprod, a, ab);
    if (rc) return rc;
    for (size_t i = 0; i < T; ++i) {
        alphas[i] = a[i];
        alpha_bars[i] = ab[i];
    }
    return DLLM_OK;
}

int dllm_p_sample_coeffs(const float *betas, size_t T, int cumprod, int alpha_mode, const size_t *t, size_t B,
                         float *coef, int *add_noise) {
    if (T == 0) return fail(DLLM_ERR_INVALID_PARAMS, "empty schedule (betas.len() - 1 underflows, lib.rs:1169)");
    if (!betas || (B && (!t || !coef))) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (alpha_mode != DLLM_ALPHA_PER_SAMPLE && alpha_mode != DLLM_ALPHA_LITERAL)
        return fail(DLLM_ERR_INVALID_PARAMS, "alpha_mode must be DLLM_ALPHA_PER_SAMPLE or DLLM_ALPHA_LITERAL");
    if (alpha_mode == DLLM_ALPHA_LITERAL && B != T)
        return fail(DLLM_ERR_INVALID_PARAMS, "literal alphas broadcast only when batch == num_timesteps (lib.rs:1191)");
    std::vector<float> a, ab;
    const int rc = alpha_tables(betas, T, cumprod, a, ab);
    if (rc) return rc;
    for (size_t i = 0; i < B; ++i) {
        const size_t ti = std::min(t[i], T - 1);
        const float abar_t = ab[ti], beta_t = betas[ti];
        const float alpha = alpha_mode == DLLM_ALPHA_LITERAL ? a[i] : a[ti];
        const float prev = ti > 0 ? ab[ti - 1] : 1.0f;
        coef[3 * i + 0] = (std::sqrt(prev) * beta_t) / (1.0f - abar_t);
        coef[3 * i + 1] = (std::sqrt(alpha) * (1.0f - prev)) / (1.0f - abar_t);
        coef[3 * i + 2] = std::sqrt(((1.0f - prev) / (1.0f - abar_t)) * beta_t);
    }
    if (add_noise) *add_noise = B > 0 && t[0] > 0;   // lib.rs:1198: decided by t[0] alone
    return DLLM_OK;
}

int dllm_add_noise_coeffs(const float *betas, size_t T, int cumprod, const size_t *t, size_t B, float *coef) {
    if (T == 0) return fail(DLLM_ERR_INVALID_PARAMS, "empty schedule (alpha_bars.len() - 1 underflows)");
    if (!betas || (B && (!t || !coef))) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    std::vector<float> a, ab;
    const int rc = alpha_tables(betas, T, cumprod, a, ab);
    if (rc) return rc;
    for (size_t i = 0; i < B; ++i) {
        const size_t ti = std::min(t[i], T - 1);
        coef[2 * i + 0] = std::sqrt(ab[ti]);
        coef[2 * i + 1] = std::sqrt(1.0f - ab[ti]);
    }
    return DLLM_OK;
}

int dllm_p_losses_coeffs(const float *betas, size_t T, const size_t *t, size_t B, float *coef) {
    if (T == 0) return fail(DLLM_ERR_INVALID_PARAMS, "empty schedule");
    if (!betas || (B && (!t || !coef))) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    for (size_t i = 0; i < B; ++i)   // alpha_bars[t] panics (lib.rs:645): no clamp here
        if (t[i] >= T) return fail(DLLM_ERR_INVALID_PARAMS, "timestep out of range of the schedule (lib.rs:645)");
    return dllm_add_noise_coeffs(betas, T, DLLM_ABAR_INCLUSIVE, t, B, coef);
}

size_t dllm_noise_mse_workspace(size_t B, size_t n) { return B * mse_chunks(n) * sizeof(float); }

int dllm_noise_mse(const void *pred, int pred_dtype, const float *noise, size_t B, size_t n, uint64_t seed,
                   uint64_t offset, float *loss, void *workspace, size_t workspace_bytes, dllm_stream_t stream) {
    if (pred_dtype != DLLM_F32 && pred_dtype != DLLM_F16)
        return fail(DLLM_ERR_UNSUPPORTED, "pred_dtype must be DLLM_F32 or DLLM_F16");
    if (B == 0) return DLLM_OK;
    if (n == 0) return fail(DLLM_ERR_INVALID_PARAMS, "the mean over an empty sample is undefined");
    if (n % 4) return fail(DLLM_ERR_UNSUPPORTED, "n must be a multiple of 4");
    if (!noise && offset % 4) return fail(DLLM_ERR_INVALID_PARAMS, "offset must be a multiple of 4");
    if (!pred || !loss || !workspace) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(noise) | reinterpret_cast<uintptr_t>(loss) |
         reinterpret_cast<uintptr_t>(workspace)) % 16)
        return fail(DLLM_ERR_INVALID_PARAMS, "pred, noise, loss and workspace must be 16-byte aligned");
    if (workspace_bytes < dllm_noise_mse_workspace(B, n))
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace smaller than dllm_noise_mse_workspace(B, n)");
    const size_t C = mse_chunks(n);
    if (C > 0x7fffffffu / B) return fail(DLLM_ERR_UNSUPPORTED, "B * ceil(n / 16384) exceeds the grid limit");
    const unsigned grid = static_cast<unsigned>(B * C);
    float *partial = static_cast<float *>(workspace);
    hipStream_t st = as_stream(stream);
    if (pred_dtype == DLLM_F16)
        launch_mse_chunks(static_cast<const __half *>(pred), noise, n, C, seed, offset, partial, loss, grid, st);
    else
        launch_mse_chunks(static_cast<const float *>(pred), noise, n, C, seed, offset, partial, loss, grid, st);
    DLLM_LAUNCH_CHECK();
    if (C > 1) {
        noise_mse_finish_kernel<<<static_cast<unsigned>(B), kMseLanes, 0, st>>>(partial, n, C, loss);
        DLLM_LAUNCH_CHECK();
    }
    return DLLM_OK;
}

int dllm_randn(uint64_t seed, uint64_t offset, float *out, size_t n, dllm_stream_t stream) {
    if (n == 0) return DLLM_OK;
    if (!out) return fail(DLLM_ERR_INVALID_PARAMS, "out is NULL");
    if (offset % 4) return fail(DLLM_ERR_INVALID_PARAMS, "offset must be a multiple of 4");
    if (reinterpret_cast<uintptr_t>(out) % 16) return fail(DLLM_ERR_INVALID_PARAMS, "out must be 16-byte aligned");
    randn_kernel<<<elem_grid(n), 256, 0, as_stream(stream)>>>(seed, offset, n, out);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

int dllm_p_sample(const float *x_t, const float *eps, const float *noise, const float *coef, size_t B, size_t D,
                  int add_noise, uint64_t seed, uint64_t offset, float *x_prev, dllm_stream_t stream) {
    const size_t n = B * D;
    if (n == 0) return DLLM_OK;
    if (!x_t || !eps || !coef || !x_prev) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (!noise && offset % 4) return fail(DLLM_ERR_INVALID_PARAMS, "offset must be a multiple of 4");
    if ((reinterpret_cast<uintptr_t>(x_t) | reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(x_prev)) % 16)
        return fail(DLLM_ERR_INVALID_PARAMS, "x_t, eps and x_prev must be 16-byte aligned");
    p_sample_kernel<<<elem_grid(n), 256, 0, as_stream(stream)>>>(x_t, eps, noise, coef, n, D, add_noise ? 1 : 0,
                                                                 seed, offset, x_prev);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

int dllm_add_noise(const float *x0, const float *noise, const float *coef, size_t B, size_t D, uint64_t seed,
                   uint64_t offset, float *noisy, float *noise_out, dllm_stream_t stream) {
    const size_t n = B * D;
    if (n == 0) return DLLM_OK;
    if (!x0 || !coef || !noisy) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (!noise && offset % 4) return fail(DLLM_ERR_INVALID_PARAMS, "offset must be a multiple of 4");
    add_noise_kernel<<<elem_grid(n), 256, 0, as_stream(stream)>>>(x0, noise, coef, n, D, seed, offset, noisy,
                                                                  noise_out);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

}  // extern "C"
