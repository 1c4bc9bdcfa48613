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
// and token sampling (8j): temperature, top-k and three seeded picks (chunk, lane, element) per row.
//   token_select_kernel  one block per row, only when 0 < top_k < V: the threshold tau by a radix select
//   token_chunk_kernel   the same kernel, its element transform y = RN(x r), -inf below tau
//   token_pick_kernel    one block per row: the pieces combined, the chunk picked and read again, the
//                        lane and the element picked, token and {m, Z, p_token} written
// Top-p and min-p (8k) are one more question about the same threshold:
//   token_nucleus_kernel one block per row, only when top_p < 1 or min_p > 0, after the select: m, then a
//                        radix select over u64 weight sums; the combined tau replaces the select's
// No global atomics, no allocation, no synchronisation.
#include "common.hpp"
#include "token_args.hpp"
#include "token_exp.hpp"
#include "token_nucleus_rule.hpp"
#include "token_sample_rule.hpp"

#include <limits>

namespace dllm {
namespace {

constexpr int kTokLanes = 256;                         // lanes of a chunk = threads of a block
constexpr int kTokTrips = 16;                          // groups of four per lane and chunk
static_assert(kTokChunk == 4 * kTokLanes * kTokTrips, "a chunk (token_args.hpp) is 16384 elements");
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

// The element transform of the chunk pass.  The readout reads the logits as they are; the sampler
// (8j.1, 8j.2) reads y = RN(x r) with everything below the row's threshold tau turned into -inf
// (tau == -inf masks nothing; a NaN compares false and stays a NaN).
struct TokIdentity {
    static constexpr bool kSample = false;
    __device__ float tau(size_t) const { return 0.f; }
    __device__ float operator()(float v, float) const { return v; }
};
struct TokTempered {
    static constexpr bool kSample = true;
    float r;
    const float *taus;   // [M], or NULL when nothing is masked
    __device__ float tau(size_t b) const { return taus ? taus[b] : tok_ninf(); }
    __device__ float operator()(float v, float tau) const {
        const float y = v * r;
        return y < tau ? tok_ninf() : y;
    }
};

template <typename Xf>
__device__ __forceinline__ void tok_transform(float4 (&x)[kTokTrips], const Xf &xf, float tau) {
#pragma unroll
    for (int k = 0; k < kTokTrips; ++k) {
        x[k].x = xf(x[k].x, tau);
        x[k].y = xf(x[k].y, tau);
        x[k].z = xf(x[k].z, tau);
        x[k].w = xf(x[k].w, tau);
    }
}

// The chunk of block-uniform index c of `row` in the lane's registers: all 16 loads in flight before
// the first use; -inf at an index >= V.  (The pick pass's loads.  The chunk kernel spells the same two
// loops out: through this helper hipcc emits another schedule for the identity instantiation than the
// one the readout's record was measured with.)
template <typename T>
__device__ __forceinline__ void tok_load_chunk(float4 (&x)[kTokTrips], const T *__restrict__ row, size_t i0, bool full,
                                               size_t V) {
    if (full) {
#pragma unroll
        for (int k = 0; k < kTokTrips; ++k) x[k] = tok_load4(row + i0 + static_cast<size_t>(k) * (4 * kTokLanes));
    } else {
#pragma unroll
        for (int k = 0; k < kTokTrips; ++k) x[k] = tok_group(row, i0 + static_cast<size_t>(k) * (4 * kTokLanes), V);
    }
}

// Block (b, c) = blockIdx.x: chunk c of row b -> part[b C + c]; for a one-chunk row of the readout,
// whose row values are the piece's, tokens[b] and stats[b] directly.
template <typename T, typename Xf>
__global__ void __launch_bounds__(kTokLanes) token_chunk_kernel(const T *__restrict__ logits, size_t V, size_t ld,
                                                                size_t C, TokPiece *__restrict__ part,
                                                                int32_t *__restrict__ tokens,
                                                                float *__restrict__ stats, const Xf xf) {
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

    if constexpr (Xf::kSample) tok_transform(x, xf, xf.tau(b));

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
        if (C == 1 && !Xf::kSample) {
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

// ---- token sampling (include/dllm_quant.h 8j) ------------------------------------------------------

// The monotone u32 key of a non-NaN f32 (-0 counts as +0): a larger value has a larger key.
__device__ __forceinline__ uint32_t tok_key(float y) {
    uint32_t b = __float_as_uint(y);
    b = b == 0x80000000u ? 0u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float tok_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

constexpr int kSelBins = 2048;                          // 11 bits; the last pass uses the lower 1024
constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelCopies = 4;                           // copies of every bin, one per lane mod 4
constexpr int kSelPer = kSelBins / kSelThreads;         // bins per thread in the rank search

// Block b: taus[b] = the top_k-th largest y = RN(x r) of row b (0 < top_k < V), by a radix select on
// the key: digits of 11, 11 and 10 bits from the top, one histogram in LDS per pass (integer atomics:
// the counts do not depend on the order), the rank walked down from the largest digit.  The counts are
// exact, so tau is the value 8j.2 defines whatever the order of arrival.  Logits crowd into a few
// exponents, so the first digit's counts crowd into a few bins: every bin has four copies in adjacent
// banks, lane l adds to copy l mod 4, and a wave's adds to one bin meet four at a time fewer.  A NaN's
// key falls into some bin: such a row is degenerate whatever tau comes out.  Passes two and three
// re-read the row (L2).
template <typename T>
__global__ void __launch_bounds__(kSelThreads) token_select_kernel(const T *__restrict__ logits, size_t V, size_t ld,
                                                                   float r, uint32_t top_k, float *__restrict__ taus) {
    __shared__ uint32_t hist[kSelBins * kSelCopies];
    __shared__ uint32_t w_tot[kSelWaves];
    __shared__ uint32_t sel[2];                          // the digit found, and the rank left inside it
    const T *row = logits + blockIdx.x * ld;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid / 64;
    uint32_t *mine = hist + (lane & (kSelCopies - 1));
    uint32_t prefix = 0, himask = 0, k = top_k;
    if (tid < 2) sel[tid] = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const uint32_t dmask = pass == 2 ? 1023u : 2047u;
        for (int i = tid; i < kSelBins * kSelCopies; i += kSelThreads) hist[i] = 0;
        __syncthreads();
        const auto count = [&](float x) {
            const uint32_t key = tok_key(x * r);
            if ((key & himask) == prefix) atomicAdd(&mine[kSelCopies * ((key >> shift) & dmask)], 1u);
        };
        const auto count4 = [&](const float4 &v) { count(v.x), count(v.y), count(v.z), count(v.w); };
        // the groups of four inside the row, four loads in flight; then the row's last one to three elements
        const size_t G = V / 4;
        size_t g = tid;
        for (; g + 3 * kSelThreads < G; g += 4 * kSelThreads) {
            float4 v[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) v[n] = tok_load4(row + 4 * (g + static_cast<size_t>(n) * kSelThreads));
#pragma unroll
            for (int n = 0; n < 4; ++n) count4(v[n]);
        }
        for (; g < G; g += kSelThreads) count4(tok_load4(row + 4 * g));
        if (4 * G + tid < V) count(tok_widen(row[4 * G + tid]));
        __syncthreads();
        // thread t owns bins 2047 - 2 t and 2046 - 2 t: an inclusive scan over t counts from the top
        uint32_t cnt[kSelPer], ps = 0;
#pragma unroll
        for (int i = 0; i < kSelPer; ++i) {
            const uint32_t *h = hist + kSelCopies * (kSelBins - 1 - (kSelPer * tid + i));
            cnt[i] = h[0] + h[1] + h[2] + h[3];
            ps += cnt[i];
        }
        uint32_t incl = ps;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            incl += lane >= o ? up : 0u;
        }
        if (lane == 63) w_tot[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += w_tot[w];
        uint32_t above = incl - ps;
        if (above < k && k <= incl) {                    // exactly one thread: the k-th largest lies in its bins
#pragma unroll
            for (int i = 0; i < kSelPer; ++i) {
                if (above < k && k <= above + cnt[i]) {
                    sel[0] = static_cast<uint32_t>(kSelBins - 1 - (kSelPer * tid + i));
                    sel[1] = k - above;
                }
                above += cnt[i];
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        himask |= dmask << shift;
        k = sel[1];
        __syncthreads();                                 // sel and hist are rewritten by the next pass
    }
    if (tid == 0) taus[blockIdx.x] = tok_unkey(prefix);
}

// ---- top-p and min-p (include/dllm_quant.h 8k) -----------------------------------------------------

constexpr int kNucBins = 2048;                          // 11 bits; the last pass uses the lower 1024
constexpr int kNucThreads = 1024;
constexpr int kNucWaves = kNucThreads / 64;
constexpr int kNucCopies = 4;                           // copies of every bin, one per lane mod 4
constexpr int kNucPer = kNucBins / kNucThreads;         // bins per thread in the walk
constexpr uint32_t kNucKeyNinf = 0x007fffffu;           // tok_key(-inf): below the key of every other non-NaN value

// f(v) for every group of four of the row, each exactly once, two loads in flight; the elements of the
// last group that lie at or past V are -inf and are never read.  The trip counts depend on V alone.
template <typename T, typename F>
__device__ __forceinline__ void nuc_for_each(const T *__restrict__ row, size_t V, int tid, const F &f) {
    constexpr size_t step = 4 * kNucThreads;
    size_t i = 4 * static_cast<size_t>(tid);
    for (; i + step + 4 <= V; i += 2 * step) {
        const float4 a = tok_load4(row + i), b = tok_load4(row + i + step);
        f(a);
        f(b);
    }
    for (; i < V; i += step) f(tok_group(row, i, V));   // at most two trips
}

// Block b: the combined threshold of 8k.5 into taus[b], which on entry holds the top-k threshold of
// token_select_kernel when has_k (else nothing).  One read of the row for m (and whether the row is
// degenerate); then, when top-p is on, a radix select on the key of y as in token_select_kernel --
// digits of 11, 11 and 10 bits from the top -- whose bins hold u64 sums of the weights W (8k.2) instead
// of counts: integer LDS atomics, so a bin's sum does not depend on the order of arrival.  The bins are
// walked from the largest digit until the mass reaches `need` (token_nucleus_rule.hpp: the 96-bit
// comparison of 8k.3 folded into one u64 per row); a bin of weight 0 never decides, so the value found
// is one of the row's.  The first pass pays EXP for every element and also yields T (the walk's grand
// total) and the min-p minimum; the later passes pay it only for elements under the prefix found so
// far.  Four copies of every bin, one per lane mod 4, as in the select: 64 KiB of LDS, two blocks per
// CU, which is the CU's 32 waves (8 per SIMD: the launch bound asks for the 64 VGPRs that takes).
// A degenerate row (a NaN, m = +-inf) runs the same passes, adds nothing to any bin and ends with
// tau = -inf: no trip count depends on the data.
template <typename T>
__global__ void __launch_bounds__(kNucThreads, 8) token_nucleus_kernel(const T *__restrict__ logits, size_t V, size_t ld,
                                                                    float r, int has_k, int p_on, uint64_t pfix,
                                                                    uint64_t mfix, float *__restrict__ taus) {
    __shared__ unsigned long long hist[kNucBins * kNucCopies];
    __shared__ unsigned long long w_tot[kNucWaves];
    __shared__ unsigned long long sel_rem;               // the mass still to reach inside the digit found
    __shared__ uint32_t sel_bin;                         // the digit found
    __shared__ float w_m[kNucWaves];
    __shared__ int w_nan[kNucWaves];
    __shared__ uint32_t w_min[kNucWaves];
    const T *row = logits + blockIdx.x * ld;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid / 64;

    // the row maximum of y = RN(x r) over the non-NaN elements, and whether there is a NaN
    float m = tok_ninf();
    bool nan = false;
    nuc_for_each(row, V, tid, [&](const float4 &v) {
        const float y[4] = {v.x * r, v.y * r, v.z * r, v.w * r};
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            nan |= y[l] != y[l];
            m = y[l] > m ? y[l] : m;
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        m = om > m ? om : m;
    }
    const int wave_nan = __any(nan);
    if (lane == 0) {
        w_m[wave] = m;
        w_nan[wave] = wave_nan;
    }
    if (tid == 0) {
        sel_bin = 0;
        sel_rem = 0;
    }
    __syncthreads();
    int any_nan = 0;
#pragma unroll
    for (int w = 0; w < kNucWaves; ++w) {
        m = w_m[w] > m ? w_m[w] : m;
        any_nan |= w_nan[w];
    }
    m = m + 0.0f;
    const bool ok = !any_nan && m != tok_ninf() && m != std::numeric_limits<float>::infinity();
    const float tau_k = has_k ? taus[blockIdx.x] : tok_ninf();

    unsigned long long *mine = hist + (lane & (kNucCopies - 1));
    uint32_t prefix = 0, himask = 0, minkey = 0xffffffffu;
    unsigned long long need = 0;
    // unrolled: inside a rolled loop hipcc keeps the loop-invariant addresses, shuffle offsets and EXP
    // constants of all passes in registers (89 VGPRs, one block per CU); unrolled it takes 51-53
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const uint32_t dmask = pass == 2 ? 1023u : 2047u;
        if (p_on) {
            for (int i = tid; i < kNucBins * kNucCopies; i += kNucThreads) hist[i] = 0;
            __syncthreads();
        }
        nuc_for_each(row, V, tid, [&](const float4 &v) {
            const float y[4] = {v.x * r, v.y * r, v.z * r, v.w * r};
            uint32_t key[4];
            bool live[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                key[l] = tok_key(y[l]);
                live[l] = ok && (key[l] & himask) == prefix && y[l] >= tau_k;   // !ok is block-uniform
            }
            if (!(live[0] || live[1] || live[2] || live[3])) return;   // EXP only under the prefix found so far
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const float g = token::exp_le0_nonan(live[l] ? y[l] - m : tok_ninf());
                const unsigned long long W = token::nucleus_weight(g);   // 0 for an element that is not live
                minkey = mfix && W >= mfix && key[l] < minkey ? key[l] : minkey;
                if (p_on && W) atomicAdd(&mine[kNucCopies * ((key[l] >> shift) & dmask)], W);
            }
        });
        if (!p_on) break;                                // min-p alone: one pass, no histogram
        __syncthreads();
        // thread t owns bins 2047 - 2 t and 2046 - 2 t: an inclusive scan over t sums from the top
        unsigned long long sum[kNucPer], ps = 0;
#pragma unroll
        for (int i = 0; i < kNucPer; ++i) {
            const unsigned long long *h = hist + kNucCopies * (kNucBins - 1 - (kNucPer * tid + i));
            sum[i] = h[0] + h[1] + h[2] + h[3];
            ps += sum[i];
        }
        unsigned long long incl = ps;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(incl, o, 64);
            incl += lane >= o ? up : 0ull;
        }
        if (lane == 63) w_tot[wave] = incl;
        __syncthreads();
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < kNucWaves; ++w) {
            incl += w < wave ? w_tot[w] : 0ull;
            total += w_tot[w];
        }
        if (pass == 0) need = token::nucleus_need(pfix, total);   // total is T: every element took part
        unsigned long long above = incl - ps;
        if (above < need && need <= incl) {              // exactly one thread: the mass is reached in its bins
#pragma unroll
            for (int i = 0; i < kNucPer; ++i) {
                if (above < need && need <= above + sum[i]) {
                    sel_bin = static_cast<uint32_t>(kNucBins - 1 - (kNucPer * tid + i));
                    sel_rem = need - above;
                }
                above += sum[i];
            }
        }
        __syncthreads();
        prefix |= sel_bin << shift;
        himask |= dmask << shift;
        need = sel_rem;
        __syncthreads();                                 // sel_* and hist are rewritten by the next pass
    }

    // the min-p minimum over the block (the first pass saw every element)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ok_ = __shfl_xor(minkey, o, 64);
        minkey = ok_ < minkey ? ok_ : minkey;
    }
    if (lane == 0) w_min[wave] = minkey;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 0; w < kNucWaves; ++w) minkey = w_min[w] < minkey ? w_min[w] : minkey;
        uint32_t key = has_k ? tok_key(tau_k) : kNucKeyNinf;
        if (p_on) key = prefix > key ? prefix : key;
        if (mfix) key = minkey > key ? minkey : key;
        taus[blockIdx.x] = ok ? tok_unkey(key) : tok_ninf();
    }
}

// Block b: row b's C pieces combined as token_row_kernel combines them (m; Z through lanes and tree),
// then the three picks of 8j.6.  Level 1 is thread 0's fold over the C terms w_c (left in the pieces'
// Z words).  The block then re-reads chunk c*, each lane rebuilding its sum with the adds of the chunk
// pass; level 2 is thread 0's fold over the 256 lane sums, after which the one lane j whose prefix
// F_j is the first above t knows it is j*; it does level 3 on its own registers and writes the token.
// kStats is the width of a stats row: 3 = {m, Z, p_token} (8j), 4 adds the row's threshold tau (8k).
template <typename T, int kStats>
__global__ void __launch_bounds__(kTokLanes) token_pick_kernel(const T *__restrict__ logits, size_t V, size_t ld, size_t C,
                                                               TokPiece *__restrict__ part, const TokTempered xf,
                                                               const float *__restrict__ u, uint64_t seed,
                                                               uint64_t offset, int32_t *__restrict__ tokens,
                                                               float *__restrict__ stats) {
    __shared__ float lds[kTokLanes], fold[kTokLanes];
    __shared__ float w_m[kTokWaves];
    __shared__ int w_bad[kTokWaves];
    __shared__ float sh_mc, sh_m, sh_Z, sh_u1, sh_u2;
    __shared__ long long sh_c;
    const size_t b = blockIdx.x;
    TokPiece *P = part + b * C;
    const int j = threadIdx.x;

    float m = tok_ninf();
    bool bad = false;                                    // a NaN in the row, or a chunk maximum of +inf
    for (size_t c = j; c < C; c += kTokLanes) {
        m = P[c].m > m ? P[c].m : m;
        bad |= P[c].Z != P[c].Z;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        m = om > m ? om : m;
    }
    const int wave_bad = __any(bad);
    if ((j & 63) == 0) {
        w_m[j / 64] = m;
        w_bad[j / 64] = wave_bad;
    }
    __syncthreads();
    int row_bad = 0;
#pragma unroll
    for (int w = 0; w < kTokWaves; ++w) {
        m = w_m[w] > m ? w_m[w] : m;
        row_bad |= w_bad[w];
    }
    row_bad |= m == tok_ninf() || m == std::numeric_limits<float>::infinity();

    float s = 0.f;
    if (!row_bad)
        for (size_t c = j; c < C; c += kTokLanes) {
            const float mc = P[c].m;
            const float w = mc == tok_ninf() ? 0.f : P[c].Z * token::exp_le0(mc - m);
            P[c].Z = w;                                  // the term w_c, for level 1
            s = s + w;
        }
    s = tok_tree(s, lds);                                // its barriers also publish the terms
    if (j == 0) {
        long long cs = -1;
        if constexpr (kStats == 4) stats[kStats * b + 3] = row_bad ? tok_nan() : xf.tau(b);
        if (row_bad) {
            tokens[b] = -1;
            stats[kStats * b] = stats[kStats * b + 1] = stats[kStats * b + 2] = tok_nan();
        } else {
            float uu[3];
            if (u) {
                uu[0] = u[3 * b], uu[1] = u[3 * b + 1], uu[2] = u[3 * b + 2];
            } else {
                token::sample_uniforms(seed, offset + b, uu);
            }
            float S = 0.f;
            for (size_t c = 0; c < C; ++c) S = S + P[c].Z;
            const float t = uu[0] * S;
            float F = 0.f;
            for (size_t c = 0; c < C; ++c) {
                F = F + P[c].Z;
                if (t < F) {
                    cs = static_cast<long long>(c);
                    break;
                }
            }
            stats[kStats * b] = m;
            stats[kStats * b + 1] = s;
            if (cs < 0) {
                tokens[b] = -1;
                stats[kStats * b + 2] = tok_nan();
            } else {
                sh_mc = P[cs].m;
                sh_m = m, sh_Z = s, sh_u1 = uu[1], sh_u2 = uu[2];
            }
        }
        sh_c = cs;
    }
    __syncthreads();
    if (sh_c < 0) return;                                // block-uniform
    const size_t c = static_cast<size_t>(sh_c);
    const float mc = sh_mc;

    // chunk c* again: the lane sums, by the adds of the chunk pass (the row holds no NaN)
    const T *row = logits + b * ld;
    const size_t i0 = c * kTokChunk + 4 * static_cast<size_t>(j);
    float4 x[kTokTrips];
    tok_load_chunk(x, row, i0, (c + 1) * kTokChunk <= V, V);
    const float tau = xf.tau(b);
    tok_transform(x, xf, tau);
    s = 0.f;
#pragma unroll
    for (int k = 0; k < kTokTrips; ++k) {                // the weights take the elements' registers
        x[k].x = token::exp_le0_nonan(x[k].x - mc), s = s + x[k].x;
        x[k].y = token::exp_le0_nonan(x[k].y - mc), s = s + x[k].y;
        x[k].z = token::exp_le0_nonan(x[k].z - mc), s = s + x[k].z;
        x[k].w = token::exp_le0_nonan(x[k].w - mc), s = s + x[k].w;
    }
    lds[j] = s;
    __syncthreads();
    if (j == 0) {
        float F = 0.f;
#pragma unroll 8
        for (int i = 0; i < kTokLanes; ++i) {
            F = F + lds[i];
            fold[i] = F;
        }
    }
    __syncthreads();
    const float t2 = sh_u1 * fold[kTokLanes - 1];
    if (j == 0 && !(t2 < fold[kTokLanes - 1])) {         // no lane qualifies
        tokens[b] = -1;
        stats[kStats * b + 2] = tok_nan();
    }
    if (!(t2 < fold[j]) || (j > 0 && t2 < fold[j - 1])) return;   // the fold never decreases: one lane stays

    // level 3, lane j*: its 64 elements in its own order, the fold being its own sum s
    const float t3 = sh_u2 * s;
    float F = 0.f;
    int q = -1;
#pragma unroll
    for (int k = 0; k < kTokTrips; ++k) {
        const float e[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            F = F + e[l];
            q = q < 0 && t3 < F ? 4 * k + l : q;
        }
    }
    // an index >= V has weight +0 and is never picked: the token is below V < 2^31
    const size_t tok = c * kTokChunk + 4 * (static_cast<size_t>(kTokLanes) * (q >> 2) + j) + (q & 3);
    if (q < 0 || tok >= V) {
        tokens[b] = -1;
        stats[kStats * b + 2] = tok_nan();
    } else {
        tokens[b] = static_cast<int32_t>(tok);
        stats[kStats * b + 2] = token::exp_le0_nonan(xf(tok_widen(row[tok]), tau) - sh_m) / sh_Z;
    }
}

}  // namespace
}  // namespace dllm

using namespace dllm;

extern "C" {

size_t dllm_token_readout_workspace(size_t M, size_t V) { return M * tok_chunks(V) * sizeof(TokPiece); }

int dllm_token_readout(const void *logits, int dtype, size_t M, size_t V, size_t ld, int32_t *tokens, float *stats,
                       float *probs, void *workspace, size_t workspace_bytes, dllm_stream_t stream) {
    if (int rc = token::check_logits(V, ld, dtype, false)) return rc;
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
        token_chunk_kernel<<<grid, kTokLanes, 0, st>>>(static_cast<const __half *>(logits), V, ld, C, part, tokens, stats,
                                                       TokIdentity{});
    else
        token_chunk_kernel<<<grid, kTokLanes, 0, st>>>(static_cast<const float *>(logits), V, ld, C, part, tokens, stats,
                                                       TokIdentity{});
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

size_t dllm_token_sample_workspace(size_t M, size_t V, size_t top_k) {
    return M * tok_chunks(V) * sizeof(TokPiece) + (top_k > 0 && top_k < V ? M * sizeof(float) : 0);
}

size_t dllm_token_sample_ex_workspace(size_t M, size_t V, size_t top_k, float top_p, float min_p) {
    const bool slot = (top_k > 0 && top_k < V) || top_p != 1.0f || min_p != 0.0f;
    return M * tok_chunks(V) * sizeof(TokPiece) + (slot ? M * sizeof(float) : 0);
}

}  // extern "C"

namespace {

// The launches of both sampling entry points, after their checks.  kStats = 3 is dllm_token_sample;
// kStats = 4 is dllm_token_sample_ex, whose threshold search runs between the select and the chunk pass
// when a mask of 8k is on (nucleus) and leaves the combined tau in the select's slot.
template <int kStats>
int token_sample_launch(const void *logits, int dtype, size_t M, size_t V, size_t ld, float r, size_t top_k, bool p_on,
                        uint64_t pfix, uint64_t mfix, const float *u, uint64_t seed, uint64_t offset, int32_t *tokens,
                        float *stats, void *workspace, dllm_stream_t stream) {
    const size_t C = tok_chunks(V);
    const unsigned grid = static_cast<unsigned>(M * C), rows = static_cast<unsigned>(M);
    TokPiece *part = static_cast<TokPiece *>(workspace);
    const bool masked = top_k > 0 && top_k < V, nucleus = p_on || mfix != 0;
    float *taus = masked || nucleus ? reinterpret_cast<float *>(part + M * C) : nullptr;
    const TokTempered xf{r, taus};
    hipStream_t st = as_stream(stream);
    const bool f16 = dtype == DLLM_F16;
    const __half *lh = static_cast<const __half *>(logits);
    const float *lf = static_cast<const float *>(logits);
    if (masked) {
        if (f16)
            token_select_kernel<<<rows, kSelThreads, 0, st>>>(lh, V, ld, r, static_cast<uint32_t>(top_k), taus);
        else
            token_select_kernel<<<rows, kSelThreads, 0, st>>>(lf, V, ld, r, static_cast<uint32_t>(top_k), taus);
        DLLM_LAUNCH_CHECK();
    }
    if (nucleus) {
        if (f16)
            token_nucleus_kernel<<<rows, kNucThreads, 0, st>>>(lh, V, ld, r, masked, p_on, pfix, mfix, taus);
        else
            token_nucleus_kernel<<<rows, kNucThreads, 0, st>>>(lf, V, ld, r, masked, p_on, pfix, mfix, taus);
        DLLM_LAUNCH_CHECK();
    }
    if (f16)
        token_chunk_kernel<<<grid, kTokLanes, 0, st>>>(lh, V, ld, C, part, tokens, stats, xf);
    else
        token_chunk_kernel<<<grid, kTokLanes, 0, st>>>(lf, V, ld, C, part, tokens, stats, xf);
    DLLM_LAUNCH_CHECK();
    if (f16)
        token_pick_kernel<__half, kStats><<<rows, kTokLanes, 0, st>>>(lh, V, ld, C, part, xf, u, seed, offset, tokens, stats);
    else
        token_pick_kernel<float, kStats><<<rows, kTokLanes, 0, st>>>(lf, V, ld, C, part, xf, u, seed, offset, tokens, stats);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

}  // namespace

extern "C" {

int dllm_token_sample(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature, size_t top_k,
                      const float *u, uint64_t seed, uint64_t offset, int32_t *tokens, float *stats, void *workspace,
                      size_t workspace_bytes, dllm_stream_t stream) {
    float r;
    if (int rc = token::check_sample_args(V, ld, dtype, temperature, r)) return rc;
    if (M == 0) return DLLM_OK;
    if (!logits || !tokens || !stats || !workspace) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(workspace) % 4)
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace must be 4-byte aligned");
    if (workspace_bytes < dllm_token_sample_workspace(M, V, top_k))
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace smaller than dllm_token_sample_workspace(M, V, top_k)");
    if (tok_chunks(V) > 0x7fffffffu / M) return fail(DLLM_ERR_UNSUPPORTED, "M * ceil(V / 16384) exceeds the grid limit");
    return token_sample_launch<3>(logits, dtype, M, V, ld, r, top_k, false, 0, 0, u, seed, offset, tokens, stats,
                                  workspace, stream);
}

int dllm_token_sample_ex(const void *logits, int dtype, size_t M, size_t V, size_t ld, float temperature, size_t top_k,
                         float top_p, float min_p, const float *u, uint64_t seed, uint64_t offset, int32_t *tokens,
                         float *stats, void *workspace, size_t workspace_bytes, dllm_stream_t stream) {
    float r;
    if (int rc = token::check_sample_ex_args(V, ld, dtype, temperature, top_p, min_p, r)) return rc;
    if (M == 0) return DLLM_OK;
    if (!logits || !tokens || !stats || !workspace) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(workspace) % 4)
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace must be 4-byte aligned");
    if (workspace_bytes < dllm_token_sample_ex_workspace(M, V, top_k, top_p, min_p))
        return fail(DLLM_ERR_INVALID_PARAMS,
                    "workspace smaller than dllm_token_sample_ex_workspace(M, V, top_k, top_p, min_p)");
    if (tok_chunks(V) > 0x7fffffffu / M) return fail(DLLM_ERR_UNSUPPORTED, "M * ceil(V / 16384) exceeds the grid limit");
    return token_sample_launch<4>(logits, dtype, M, V, ld, r, top_k, top_p != 1.0f, token::nucleus_pfix(top_p),
                                  token::nucleus_mfix(min_p), u, seed, offset, tokens, stats, workspace, stream);
}

}  // extern "C"
