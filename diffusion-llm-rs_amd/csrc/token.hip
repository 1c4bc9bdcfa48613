// token.hip -- the token readout (include/dllm_quant.h 8h): the step from logits [M][V] to tokens.
// Per row: the greedy token (the fold of diffusion_prefill/src/lib.rs:162-174 sample_token, stated
// on the logits), stats = {m, Z} (the row maximum and the softmax denominator, so that the greedy
// token's probability is 1 / Z) and, on request, the probabilities (:141-159 predict_next_token's
// "Convert logits to probabilities").  One HBM read of the logits gives token and stats; the
// summation order is 8f's, EXP is csrc/token_exp.hpp, so the bits depend on the row alone.
//
//   token_chunk_kernel   one block of 256 per (row, chunk of 16384): the chunk in registers, two
//                        block reductions (last NaN + maximum; then sum + best), a piece per chunk
//   token_row_kernel     one block per row: the pieces combined in order, Z through the same tree
//   token_probs_kernel   p = EXP(x - m) / Z, elementwise, one block per (row, chunk)
// No atomics, no allocation, no synchronisation.
#include "common.hpp"
#include "token_exp.hpp"

#include <limits>

namespace dllm {
namespace {

constexpr int kTokLanes = 256;                         // lanes of a chunk = threads of a block
constexpr int kTokTrips = 16;                          // groups of four per lane and chunk
constexpr size_t kTokChunk = 4 * kTokLanes * kTokTrips;    // 16384 elements
constexpr int kTokWaves = kTokLanes / 64;

inline size_t tok_chunks(size_t V) { return (V + kTokChunk - 1) / kTokChunk; }

// What a chunk leaves for the row kernel: five words per (row, chunk).
struct TokPiece {
    float m;       // maximum of the chunk's non-NaN elements (a zero maximum is +0), -inf if none
    float Z;       // sum of EXP(x - m) in the pinned order; +0 when m == -inf; NaN when n >= 0 or m == +inf
    float bv;      // the best value after the chunk's last NaN ...
    int32_t bi;    // ... and its row index (the largest among equals); -1 when nothing follows the NaN
    int32_t n;     // row index of the chunk's last NaN, -1 if none
};
static_assert(sizeof(TokPiece) == 20, "dllm_token_readout_workspace counts 20 bytes per piece");

__device__ __forceinline__ float tok_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }
__device__ __forceinline__ float tok_ninf() { return -std::numeric_limits<float>::infinity(); }

__device__ __forceinline__ float tok_widen(float v) { return v; }
__device__ __forceinline__ float tok_widen(__half v) { return __half2float(v); }

// A group of four with one load.  The pointer is only element-aligned (rows of an odd ld start
// anywhere): a global load needs no more alignment than the compiler is told of, so this is one
// global_load_dwordx4 (f32) or _dwordx2 (f16) for every row layout; in a row that is not aligned to
// the group size a group now and then straddles two cache lines, and that is all the difference.
__device__ __forceinline__ float4 tok_load4(const float *p) {
    float4 v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}
__device__ __forceinline__ float4 tok_load4(const __half *p) {
    uint2 r;
    __builtin_memcpy(&r, p, sizeof(r));
    const __half2 lo = *reinterpret_cast<const __half2 *>(&r.x), hi = *reinterpret_cast<const __half2 *>(&r.y);
    return make_float4(__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi));
}
__device__ __forceinline__ void tok_store4(float *p, const float4 v) { __builtin_memcpy(p, &v, sizeof(v)); }

// The group of four at row index i (a multiple of 4): one load when the group lies inside the row,
// else element by element; nothing at or past V is ever read (-inf there: no maximum, EXP gives +0).
template <typename T>
__device__ __forceinline__ float4 tok_group(const T *__restrict__ row, size_t i, size_t V) {
    if (i + 4 <= V) return tok_load4(row + i);
    float4 v;
    v.x = i < V ? tok_widen(row[i]) : tok_ninf();
    v.y = i + 1 < V ? tok_widen(row[i + 1]) : tok_ninf();
    v.z = i + 2 < V ? tok_widen(row[i + 2]) : tok_ninf();
    v.w = i + 3 < V ? tok_widen(row[i + 3]) : tok_ninf();
    return v;
}

// The halving tree of 8f over the block's 256 lane sums: s[j] = s[j] + s[j + h], j < h, h = 128 ... 1.
// The root is thread 0's return value.
__device__ __forceinline__ float tok_tree(float s, float *lds) {
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

// Unordered "better" on (value, index) over non-NaN values: the larger value, among equals (-0 == +0)
// the larger index; index -1 is "none".
__device__ __forceinline__ void tok_better(float &bv, int &bi, float ov, int oi) {
    const bool take = oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi));
    bv = take ? ov : bv;
    bi = take ? oi : bi;
}

// Ordered combine of two adjacent pieces (left, right) of the reference's fold: a right piece with a
// NaN replaces the left one; otherwise the better best wins and ties go to the right.
__device__ __forceinline__ void tok_append(int &n, float &bv, int &bi, int rn, float rbv, int rbi) {
    if (rn >= 0) {
        n = rn;
        bv = rbv;
        bi = rbi;
    } else if (rbi >= 0 && (bi < 0 || !(bv > rbv))) {
        bv = rbv;
        bi = rbi;
    }
}

__device__ __forceinline__ void tok_write_row(int32_t *tokens, float *stats, size_t b, int n, int bi, float m, float Z) {
    tokens[b] = bi >= 0 ? bi : n;
    stats[2 * b] = n >= 0 ? tok_nan() : m;
    stats[2 * b + 1] = n >= 0 ? tok_nan() : Z;
}

// Block (b, c) = blockIdx.x: chunk c of row b -> part[b C + c]; for a one-chunk row, whose row
// values are the piece's, tokens[b] and stats[b] directly.
template <typename T>
__global__ void __launch_bounds__(kTokLanes) token_chunk_kernel(const T *__restrict__ logits, size_t V, size_t ld,
                                                                size_t C, TokPiece *__restrict__ part,
                                                                int32_t *__restrict__ tokens,
                                                                float *__restrict__ stats) {
    __shared__ float lds[kTokLanes];
    __shared__ float w_m[kTokWaves], w_bv[kTokWaves];
    __shared__ int w_n[kTokWaves], w_bi[kTokWaves], w_nan[kTokWaves];
    const size_t b = blockIdx.x / C, c = blockIdx.x % C;
    const T *row = logits + b * ld;
    const size_t i0 = c * kTokChunk + 4 * static_cast<size_t>(threadIdx.x);   // this lane's group of trip 0
    const int wave = threadIdx.x / 64;

    const bool full = (c + 1) * kTokChunk <= V;        // block-uniform: no element of the chunk is missing

    // the chunk: all 16 loads of the lane in flight before the first use
    float4 x[kTokTrips];
    if (full) {
#pragma unroll
        for (int k = 0; k < kTokTrips; ++k) x[k] = tok_load4(row + i0 + static_cast<size_t>(k) * (4 * kTokLanes));
    } else {
#pragma unroll
        for (int k = 0; k < kTokTrips; ++k) x[k] = tok_group(row, i0 + static_cast<size_t>(k) * (4 * kTokLanes), V);
    }

    // pass A: the maximum of the non-NaN elements, and whether there is a NaN at all
    float m = tok_ninf();
    bool nan = false;
#pragma unroll
    for (int k = 0; k < kTokTrips; ++k) {
        const float v[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            nan |= v[l] != v[l];
            m = v[l] > m ? v[l] : m;               // a NaN compares false
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        m = om > m ? om : m;
    }
    const int wave_nan = __any(nan);
    if ((threadIdx.x & 63) == 0) {
        w_m[wave] = m;
        w_nan[wave] = wave_nan;
    }
    __syncthreads();
    int any_nan = 0;
#pragma unroll
    for (int w = 0; w < kTokWaves; ++w) {
        m = w_m[w] > m ? w_m[w] : m;
        any_nan |= w_nan[w];
    }
    m = m + 0.0f;                                  // a zero maximum is +0

    // the index of the last NaN: only a chunk that holds one pays for the search (block-uniform)
    int n = -1;
    if (any_nan) {
#pragma unroll
        for (int k = 0; k < kTokTrips; ++k) {
            const uint32_t i = static_cast<uint32_t>(i0) + k * (4 * kTokLanes);   // exact wherever an element exists
            const float v[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
            for (int l = 0; l < 4; ++l) n = v[l] != v[l] ? static_cast<int>(i + l) : n;   // ascending within the lane
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int on = __shfl_xor(n, o, 64);
            n = on > n ? on : n;
        }
        if ((threadIdx.x & 63) == 0) w_n[wave] = n;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kTokWaves; ++w) n = w_n[w] > n ? w_n[w] : n;
    }

    // pass B: the sum of EXP(x - m) in the pinned order, and the best element after the last NaN
    float s = 0.f, bv = tok_ninf();
    int bi = -1;
    if (full && !any_nan) {
        // the best value is m itself: only the lane's last element equal to it is looked for
        int li = -1;
#pragma unroll
        for (int k = 0; k < kTokTrips; ++k) {
            const float v[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                s = s + token::exp_le0_nonan(v[l] - m);
                li = v[l] == m ? 4 * k + l : li;
            }
        }
        bv = m;
        bi = li >= 0 ? static_cast<int>(i0) + (li >> 2) * (4 * kTokLanes) + (li & 3) : -1;
    } else {
#pragma unroll
        for (int k = 0; k < kTokTrips; ++k) {
            if (c * kTokChunk + static_cast<size_t>(k) * (4 * kTokLanes) >= V) break;   // block-uniform: +0 terms only
            const size_t ik = i0 + static_cast<size_t>(k) * (4 * kTokLanes);
            const float v[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                s = s + token::exp_le0(v[l] - m);
                const int idx = static_cast<int>(static_cast<uint32_t>(ik) + l);
                const bool take = ik + l < V && idx > n && !(bv > v[l]);
                bv = take ? v[l] : bv;
                bi = take ? idx : bi;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        tok_better(bv, bi, ov, oi);
    }
    if ((threadIdx.x & 63) == 0) {
        w_bv[wave] = bv;
        w_bi[wave] = bi;
    }
    s = tok_tree(s, lds);                          // its barriers also publish w_bv / w_bi
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kTokWaves; ++w) tok_better(bv, bi, w_bv[w], w_bi[w]);
        float Z = s;
        if (m == tok_ninf()) Z = 0.f;
        if (n >= 0 || m == std::numeric_limits<float>::infinity()) Z = tok_nan();
        if (C == 1) {
            tok_write_row(tokens, stats, b, n, bi, m, Z);
        } else {
            TokPiece p;
            p.m = m, p.Z = Z, p.bv = bv, p.bi = bi, p.n = n;
            part[blockIdx.x] = p;
        }
    }
}

// Block b: row b's C pieces.  m = max m_c; the terms RN(Z_c EXP(m_c - m)) go to 256 lanes round-robin
// and through the tree; the token pieces are appended in chunk order (each lane a run of adjacent
// chunks, thread 0 the lanes' results).
__global__ void __launch_bounds__(kTokLanes) token_row_kernel(const TokPiece *__restrict__ part, size_t C,
                                                              int32_t *__restrict__ tokens, float *__restrict__ stats) {
    __shared__ float lds[kTokLanes];
    __shared__ float p_bv[kTokLanes];
    __shared__ int p_n[kTokLanes], p_bi[kTokLanes];
    __shared__ float w_m[kTokWaves];
    const TokPiece *P = part + blockIdx.x * C;
    const size_t j = threadIdx.x;

    float m = tok_ninf();
    for (size_t c = j; c < C; c += kTokLanes) m = P[c].m > m ? P[c].m : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        m = om > m ? om : m;
    }
    if ((threadIdx.x & 63) == 0) w_m[threadIdx.x / 64] = m;

    const size_t per = (C + kTokLanes - 1) / kTokLanes, runs = (C + per - 1) / per;
    int n = -1, bi = -1;
    float bv = tok_ninf();
    for (size_t c = j * per; c < C && c < (j + 1) * per; ++c) tok_append(n, bv, bi, P[c].n, P[c].bv, P[c].bi);
    p_n[j] = n, p_bv[j] = bv, p_bi[j] = bi;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kTokWaves; ++w) m = w_m[w] > m ? w_m[w] : m;

    float s = 0.f;
    if (m != std::numeric_limits<float>::infinity())   // else Z is NaN below: no inf - inf here
        for (size_t c = j; c < C; c += kTokLanes) {
            const float mc = P[c].m;
            s = s + (mc == tok_ninf() ? 0.f : P[c].Z * token::exp_le0(mc - m));
        }
    s = tok_tree(s, lds);
    if (threadIdx.x == 0) {
        for (size_t r = 1; r < runs; ++r) tok_append(n, bv, bi, p_n[r], p_bv[r], p_bi[r]);
        float Z = s;
        if (m == tok_ninf()) Z = 0.f;
        if (m == std::numeric_limits<float>::infinity()) Z = tok_nan();
        // tok_append never clears n: n >= 0 here exactly when the row holds a NaN
        tok_write_row(tokens, stats, blockIdx.x, n, bi, m, Z);
    }
}

// Block (b, c): p = RN(EXP(RN(x - m)) / Z) over chunk c of row b; the quiet NaN for every element of
// a row whose Z is NaN or whose m is -inf.  probs rows are contiguous (stride V).  Four trips of loads
// in flight per pass.
template <typename T>
__global__ void __launch_bounds__(kTokLanes) token_probs_kernel(const T *__restrict__ logits, size_t V, size_t ld,
                                                                size_t C, const float *__restrict__ stats,
                                                                float *__restrict__ probs) {
    const size_t b = blockIdx.x / C, c = blockIdx.x % C;
    const T *row = logits + b * ld;
    float *out = probs + b * V;
    const float m = stats[2 * b], Z = stats[2 * b + 1];
    const bool undefined = Z != Z || m == tok_ninf();
    const size_t i0 = c * kTokChunk + 4 * static_cast<size_t>(threadIdx.x);
    for (int k0 = 0; k0 < kTokTrips; k0 += 4) {
        if (c * kTokChunk + static_cast<size_t>(k0) * (4 * kTokLanes) >= V) break;   // block-uniform
        float4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = tok_group(row, i0 + static_cast<size_t>(k0 + k) * (4 * kTokLanes), V);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t i = i0 + static_cast<size_t>(k0 + k) * (4 * kTokLanes);
            if (i >= V) break;
            // a defined row holds no NaN and no +inf: x - m is never NaN there
            float4 p;
            p.x = undefined ? tok_nan() : token::exp_le0_nonan(x[k].x - m) / Z;
            p.y = undefined ? tok_nan() : token::exp_le0_nonan(x[k].y - m) / Z;
            p.z = undefined ? tok_nan() : token::exp_le0_nonan(x[k].z - m) / Z;
            p.w = undefined ? tok_nan() : token::exp_le0_nonan(x[k].w - m) / Z;
            if (i + 4 <= V) {
                tok_store4(out + i, p);
            } else {                                   // the row's last, ragged group
                const float pl[3] = {p.x, p.y, p.z};
                for (size_t l = 0; i + l < V; ++l) out[i + l] = pl[l];
            }
        }
    }
}

}  // namespace
}  // namespace dllm

using namespace dllm;

extern "C" {

size_t dllm_token_readout_workspace(size_t M, size_t V) { return M * tok_chunks(V) * sizeof(TokPiece); }

int dllm_token_readout(const void *logits, int dtype, size_t M, size_t V, size_t ld, int32_t *tokens, float *stats,
                       float *probs, void *workspace, size_t workspace_bytes, dllm_stream_t stream) {
    if (V == 0) return fail(DLLM_ERR_INVALID_PARAMS, "V == 0: no token to read out of an empty vocabulary");
    if (ld < V) return fail(DLLM_ERR_INVALID_PARAMS, "ld must be at least V");
    if (V >= (size_t(1) << 31)) return fail(DLLM_ERR_SHAPE_MISMATCH, "V must be below 2^31 (the token is an int32)");
    if (dtype != DLLM_F32 && dtype != DLLM_F16) return fail(DLLM_ERR_UNSUPPORTED, "dtype must be DLLM_F32 or DLLM_F16");
    if (M == 0) return DLLM_OK;
    if (!logits || !tokens || !stats || !workspace) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(workspace) % 4)
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace must be 4-byte aligned");
    if (workspace_bytes < dllm_token_readout_workspace(M, V))
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace smaller than dllm_token_readout_workspace(M, V)");
    const size_t C = tok_chunks(V);
    if (C > 0x7fffffffu / M) return fail(DLLM_ERR_UNSUPPORTED, "M * ceil(V / 16384) exceeds the grid limit");
    const unsigned grid = static_cast<unsigned>(M * C);
    TokPiece *part = static_cast<TokPiece *>(workspace);
    hipStream_t st = as_stream(stream);
    if (dtype == DLLM_F16)
        token_chunk_kernel<<<grid, kTokLanes, 0, st>>>(static_cast<const __half *>(logits), V, ld, C, part, tokens, stats);
    else
        token_chunk_kernel<<<grid, kTokLanes, 0, st>>>(static_cast<const float *>(logits), V, ld, C, part, tokens, stats);
    DLLM_LAUNCH_CHECK();
    if (C > 1) {
        token_row_kernel<<<static_cast<unsigned>(M), kTokLanes, 0, st>>>(part, C, tokens, stats);
        DLLM_LAUNCH_CHECK();
    }
    if (probs) {
        if (dtype == DLLM_F16)
            token_probs_kernel<<<grid, kTokLanes, 0, st>>>(static_cast<const __half *>(logits), V, ld, C, stats, probs);
        else
            token_probs_kernel<<<grid, kTokLanes, 0, st>>>(static_cast<const float *>(logits), V, ld, C, stats, probs);
        DLLM_LAUNCH_CHECK();
    }
    return DLLM_OK;
}

}  // extern "C"
