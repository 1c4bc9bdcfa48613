// search.hip -- exact cosine top-k over the CompressedVector store (codes u8 [rows][dim], one
// scale and zero point per row), scored on the byte codes with the dequantization folded in: the
// one consumer of dllm_compress_vectors' output that reads it on the device.
//
// The score rule (strand sums, row table, key order) is pinned in include/dllm_quant.h; this file
// is its device form, host_rules.cpp's dllm_search_*_host its plain C++ mirror and
// tests/search_ref.py its numpy restatement.  Four kernels, all on the caller's stream, no atomics,
// no allocation:
//   search_table_kernel   a wave per kTableRows rows: C1 = sum c, C2 = sum c^2 (exact u32), the f64 norm, (u, v)
//   search_query_kernel   one wave per query: Qs, 1 / sqrt(Qn)
//   search_scan_kernel    the hot path: streams the codes once per tile of kScanTile queries, one
//                         wave per kScanRows rows, lane = strand, 256 contiguous bytes per row and
//                         wave-instruction; writes scores f32 [nq][rows]
//   search_select_kernel  packs (score, index) keys, takes a slice of kSlice of them into LDS and keeps
//                         the k largest in order (a bitonic network cut off at runs of K >= k, then
//                         halved round by round); repeated over the survivors until one slice is left
// Tile and slice sizes are the ones scripts/search_time.py measured.
//
// Reference: diffusion_prefill/src/fusion_ann.rs:109-136 (cosine, sort descending, take k).
#include "common.hpp"
#include "search_rule.hpp"
#include "search_select.hpp"

#include <cmath>

namespace dllm {
namespace {

using search::search_key;   // the key order: search_rule.hpp

constexpr int kStrands = 64;            // = the wave: lane l owns the codes d with (d / 4) % 64 == l
constexpr int kTripBytes = 4 * kStrands;
constexpr int kScanRows = 8;            // rows a wave keeps in flight per pass
constexpr int kScanWaves = 4;
constexpr int kTableRows = 8;           // rows a table wave sums per pass
constexpr int kScanThreads = kScanWaves * kStrands;
constexpr int kScanTile = 4;            // queries held in registers per pass over the codes
constexpr int kSlice = 2048;            // keys one select workgroup sorts in LDS (16 KiB)
constexpr int kSelThreads = 256;

// a[i] = a[i] + a[i ^ m], m = 32 .. 1: every lane ends with the strand tree's root.
__device__ __forceinline__ float strand_tree(float a) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) a = a + __shfl_xor(a, m, 64);
    return a;
}

// The same tree over N independent sums at once, N = 8, 16 or 32 per lane.  While more than one sum
// is left a level hands half of them to the partner lane and adds the partner's half of the others:
// lane i and lane i ^ m form the same a[i] + a[i ^ m] (the addition commutes bit for bit), each for
// the sums it keeps, so a level costs N / 2, N / 4, ... shuffles instead of N.  Returns, in every
// lane, the root of sum number lane >> (6 - log2 N).
template <int N>
__device__ __forceinline__ float strand_tree_many(float (&v)[N], int lane) {
    int cnt = N;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        if (cnt > 1) {
            const bool up = (lane & m) != 0;
            const int h = cnt / 2;
#pragma unroll
            for (int i = 0; i < N / 2; ++i) {
                if (i < h) {
                    const float lo = v[i], hi = v[i + h];   // values first: a ?: of two array elements is
                    const float keep = up ? hi : lo;        // an lvalue, i.e. a run-time register index
                    const float send = up ? lo : hi;
                    v[i] = keep + __shfl_xor(send, m, 64);
                }
            }
            cnt = h;
        } else {
            v[0] = v[0] + __shfl_xor(v[0], m, 64);
        }
    }
    return v[0];
}

constexpr int ilog2(int n) { return n <= 1 ? 0 : 1 + ilog2(n / 2); }

// ---- row table -----------------------------------------------------------------------------------

__global__ void __launch_bounds__(kScanThreads) search_table_kernel(const uint8_t *__restrict__ codes, size_t rows,
                                                                    size_t dim, const float *__restrict__ scales,
                                                                    const float *__restrict__ zps, int aligned,
                                                                    float *__restrict__ table) {
    const int lane = threadIdx.x & 63;
    const size_t row0 = (static_cast<size_t>(blockIdx.x) * kScanWaves + (threadIdx.x >> 6)) * kTableRows;
    if (row0 >= rows) return;
    const uint8_t *p[kTableRows];
#pragma unroll
    for (int r = 0; r < kTableRows; ++r) {   // rows past the end re-read the last row; never stored
        const size_t row = row0 + r < rows ? row0 + r : rows - 1;
        p[r] = codes + row * dim;
    }
    uint32_t c1[kTableRows], c2[kTableRows];   // exact: dim <= 65535, so C2 <= 65535 * 255^2 < 2^32
#pragma unroll
    for (int r = 0; r < kTableRows; ++r) c1[r] = c2[r] = 0u;
    if (aligned) {
        for (size_t d = 4 * static_cast<size_t>(lane); d < dim; d += kTripBytes) {
            uint32_t w[kTableRows];
#pragma unroll
            for (int r = 0; r < kTableRows; ++r) w[r] = *reinterpret_cast<const uint32_t *>(p[r] + d);
#pragma unroll
            for (int r = 0; r < kTableRows; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t c = (w[r] >> (8 * i)) & 0xffu;
                    c1[r] += c;
                    c2[r] += c * c;
                }
        }
    } else {
        for (size_t d = lane; d < dim; d += kStrands) {
#pragma unroll
            for (int r = 0; r < kTableRows; ++r) {
                const uint32_t c = p[r][d];
                c1[r] += c;
                c2[r] += c * c;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kTableRows; ++r) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            c1[r] += __shfl_xor(c1[r], m, 64);
            c2[r] += __shfl_xor(c2[r], m, 64);
        }
        const size_t row = row0 + r;
        if (lane == r && row < rows) {
            const float sf = scales[row], zf = zps[row];
            const double s = sf, z = zf;
            const double nb2 = ((s * s) * static_cast<double>(c2[r]) + ((2.0 * s) * z) * static_cast<double>(c1[r])) +
                               (z * z) * static_cast<double>(dim);
            const float w = nb2 > 0.0 ? static_cast<float>(1.0 / sqrt(nb2)) : 0.0f;
            table[2 * row] = sf * w;
            table[2 * row + 1] = zf * w;
        }
    }
}

// ---- per query: Qs and wq ------------------------------------------------------------------------

__global__ void __launch_bounds__(kStrands) search_query_kernel(const float *__restrict__ Q, size_t dim,
                                                                float *__restrict__ qstat) {
    const int lane = threadIdx.x;
    const float *q = Q + static_cast<size_t>(blockIdx.x) * dim;
    float qs = 0.0f, qn = 0.0f;
    for (size_t base = 4 * static_cast<size_t>(lane); base < dim; base += kTripBytes) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (base + i < dim) {
                const float x = q[base + i];
                qs = fmaf(x, 1.0f, qs);
                qn = fmaf(x, x, qn);
            }
        }
    }
    qs = strand_tree(qs);
    qn = strand_tree(qn);
    if (lane == 0) {
        qstat[2 * blockIdx.x] = qs;
        qstat[2 * blockIdx.x + 1] = qn > 0.0f ? 1.0f / sqrtf(qn) : 0.0f;
    }
}

// ---- scan ----------------------------------------------------------------------------------------

// One trip: the lane's group of four codes of each of the wave's rows against the same four
// elements of each query.  GUARD: the row's last, ragged trip (elements at d >= dim count as q = 0,
// c = 0, which leaves a partial unchanged: a partial is never -0).  ALIGNED: dim % 4 == 0 with codes
// 4-byte and queries 16-byte aligned, so a group is one dword and a query group one 16-byte load.
template <int TQ, bool ALIGNED, bool GUARD>
__device__ __forceinline__ void scan_trip(const uint8_t *(&rp)[kScanRows], const float *(&qp)[TQ], size_t off,
                                          size_t dim, float (&a)[TQ * kScanRows]) {
    uint32_t c[kScanRows];
    float q[TQ][4];
    if (ALIGNED) {
        const bool in = !GUARD || off < dim;
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) c[r] = in ? *reinterpret_cast<const uint32_t *>(rp[r] + off) : 0u;
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const float4 v = in ? *reinterpret_cast<const float4 *>(qp[j] + off) : make_float4(0.f, 0.f, 0.f, 0.f);
            q[j][0] = v.x, q[j][1] = v.y, q[j][2] = v.z, q[j][3] = v.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) {
            c[r] = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (!GUARD || off + i < dim) c[r] |= static_cast<uint32_t>(rp[r][off + i]) << (8 * i);
        }
#pragma unroll
        for (int j = 0; j < TQ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) q[j][i] = (!GUARD || off + i < dim) ? qp[j][off + i] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) {
            const float f = static_cast<float>((c[r] >> (8 * i)) & 0xffu);
#pragma unroll
            for (int j = 0; j < TQ; ++j) a[j * kScanRows + r] = fmaf(q[j][i], f, a[j * kScanRows + r]);
        }
}

// grid.x: groups of kScanWaves * kScanRows rows; grid.y: tiles of TQ queries from query j0 on.
template <int TQ, bool ALIGNED>
__global__ void __launch_bounds__(kScanThreads) search_scan_kernel(const float *__restrict__ Q,
                                                                   const uint8_t *__restrict__ codes,
                                                                   const float *__restrict__ table,
                                                                   const float *__restrict__ qstat, size_t rows,
                                                                   size_t dim, size_t j0, float *__restrict__ scores) {
    constexpr int N = TQ * kScanRows;
    const int lane = threadIdx.x & 63;
    const size_t row0 = (static_cast<size_t>(blockIdx.x) * kScanWaves + (threadIdx.x >> 6)) * kScanRows;
    if (row0 >= rows) return;
    const size_t jt = j0 + static_cast<size_t>(blockIdx.y) * TQ;
    const uint8_t *rp[kScanRows];
    const float *qp[TQ];
#pragma unroll
    for (int r = 0; r < kScanRows; ++r) {   // rows past the end re-read the last row; never stored
        const size_t row = row0 + r < rows ? row0 + r : rows - 1;
        rp[r] = codes + row * dim;
    }
#pragma unroll
    for (int j = 0; j < TQ; ++j) qp[j] = Q + (jt + j) * dim;
    float a[N];
#pragma unroll
    for (int n = 0; n < N; ++n) a[n] = 0.0f;

    const size_t full = dim / kTripBytes * kTripBytes;
    size_t off = 4 * static_cast<size_t>(lane);
    for (; off < full; off += kTripBytes) scan_trip<TQ, ALIGNED, false>(rp, qp, off, dim, a);
    if (full < dim) scan_trip<TQ, ALIGNED, true>(rp, qp, off, dim, a);

    const float A = strand_tree_many<N>(a, lane);
    constexpr int SH = 6 - ilog2(N);
    if ((lane & ((1 << SH) - 1)) == 0) {
        const int n = lane >> SH;
        const size_t j = jt + n / kScanRows, row = row0 + n % kScanRows;
        if (row < rows) {
            const float u = table[2 * row], v = table[2 * row + 1];
            const float qs = qstat[2 * j], wq = qstat[2 * j + 1];
            scores[j * rows + row] = fmaf(u, A, v * qs) * wq;
        }
    }
}

// ---- select ----------------------------------------------------------------------------------------

// One stage of the bitonic network over s[0, len): element lo against lo | jj, the larger first
// where (lo & kk) == 0.  A thread's pairs are all read, then all written (taken one pair at a time,
// each LDS round trip would wait for the one before it).  Ends with a barrier.
__device__ __forceinline__ void select_stage(uint64_t *s, unsigned len, unsigned kk, unsigned jj, unsigned tid) {
    constexpr int kPairs = kSlice / 2 / kSelThreads;
    unsigned lo[kPairs];
    uint64_t x[kPairs], y[kPairs];
#pragma unroll
    for (int u = 0; u < kPairs; ++u) {
        const unsigned p = tid + u * kSelThreads;
        lo[u] = ((p & ~(jj - 1)) << 1) | (p & (jj - 1));
        x[u] = y[u] = 0;
        if (p < len / 2) x[u] = s[lo[u]], y[u] = s[lo[u] | jj];
    }
#pragma unroll
    for (int u = 0; u < kPairs; ++u) {
        if (tid + u * kSelThreads < len / 2) {
            const bool sw = ((lo[u] & kk) == 0) ? x[u] < y[u] : x[u] > y[u];
            s[lo[u]] = sw ? y[u] : x[u];
            s[lo[u] | jj] = sw ? x[u] : y[u];
        }
    }
    __syncthreads();
}

// Block (j, sl) takes elements [sl kSlice, (sl + 1) kSlice) of query j's n keys (FROM_SCORES: made
// from its score row, n == rows) and keeps the k largest in order: as keys [j][sl][k] for the next
// pass, or, when this is the only slice left (final), as the call's idx / scores [j][k].
// Only k <= K keys are wanted (K a power of two), so the slice is not sorted whole: the network
// stops at runs of K (alternately descending and ascending), then each round replaces two
// neighbouring runs by the elementwise larger of the two (a descending run followed by an ascending
// one is bitonic, so those are its K largest, again bitonic), halving the data, and re-sorts the runs
// with the log2 K merge stages.  Keys are unique, so the result is the sort's first k whatever the
// route.  DROP (with FROM_SCORES): a NaN score is no row at all (key 0), the sentinel of a producer
// whose rule never yields a NaN (neighbors.hip's dropped pairs).
template <bool FROM_SCORES, bool DROP = false>
__global__ void __launch_bounds__(kSelThreads) search_select_kernel(const float *__restrict__ scores,
                                                                    const uint64_t *__restrict__ keys_in, size_t n,
                                                                    size_t nsl, size_t rows, unsigned k,
                                                                    uint64_t *__restrict__ keys_out,
                                                                    int32_t *__restrict__ idx, float *__restrict__ out,
                                                                    int final) {
    __shared__ uint64_t s[kSlice];
    const unsigned tid = threadIdx.x;
    const size_t j = blockIdx.x / nsl, sl = blockIdx.x % nsl;
    const size_t base = sl * kSlice;
    const unsigned cnt = static_cast<unsigned>(n - base < kSlice ? n - base : kSlice);
    unsigned P = 2;                                            // a power of two >= cnt
    while (P < cnt) P <<= 1;
    unsigned K = 2;                                            // a power of two >= k, at most P
    while (K < k && K < P) K <<= 1;
    const unsigned fill = P > k ? P : k;                       // <= kSlice; keys past cnt are "no row"
    for (unsigned i = tid; i < fill; i += kSelThreads) {
        const size_t e = base + i;
        uint64_t key = 0;
        if (i < cnt) {
            if (FROM_SCORES) {
                const float sc = scores[j * rows + e];
                key = (DROP && sc != sc) ? 0 : search_key(sc, static_cast<uint32_t>(e));
            } else {
                key = keys_in[j * n + e];
            }
        }
        s[i] = key;
    }
    __syncthreads();
    for (unsigned kk = 2; kk <= K; kk <<= 1)                   // runs of K
        for (unsigned jj = kk >> 1; jj > 0; jj >>= 1) select_stage(s, P, kk, jj, tid);
    for (unsigned len = P; len > K; ) {
        constexpr int kOuts = kSlice / 2 / kSelThreads;
        uint64_t m[kOuts];
#pragma unroll
        for (int u = 0; u < kOuts; ++u) {                      // output o = run r, place i: runs 2r and 2r + 1
            const unsigned o = tid + u * kSelThreads, at = o + (o / K) * K;
            m[u] = 0;
            if (o < len / 2) {
                const uint64_t x = s[at], y = s[at + K];
                m[u] = x > y ? x : y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kOuts; ++u) {
            const unsigned o = tid + u * kSelThreads;
            if (o < len / 2) s[o] = m[u];
        }
        __syncthreads();
        len >>= 1;
        for (unsigned jj = K >> 1; jj > 0; jj >>= 1) select_stage(s, len, K, jj, tid);
    }
    for (unsigned i = tid; i < k; i += kSelThreads) {
        const uint64_t key = s[i];
        if (final) {
            const uint32_t id = ~static_cast<uint32_t>(key);
            idx[j * k + i] = key ? static_cast<int32_t>(id) : -1;
            out[j * k + i] = key ? scores[j * rows + id] : -INFINITY;
        } else {
            keys_out[(j * nsl + sl) * k + i] = key;
        }
    }
}

__global__ void search_fill_empty_kernel(size_t n, int32_t *__restrict__ idx, float *__restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) {
        idx[i] = -1;
        out[i] = -INFINITY;
    }
}

// ---- host ------------------------------------------------------------------------------------------

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
inline size_t slices_of(size_t n) { return (n + kSlice - 1) / kSlice; }

// Workspace: qstat f32 [nq][2] | scores f32 [nq][rows] | keys A u64 [nq][slices(rows)][k] | keys B
// u64 [nq][slices(slices(rows) k)][k]; the select passes alternate between A and B.
struct SearchPlan {
    size_t qstat = 0, scores = 0, keys_a = 0, keys_b = 0, total = 0;
};
SearchPlan search_plan(size_t nq, size_t rows, size_t k) {
    SearchPlan p;
    p.qstat = 0;
    p.scores = up16(nq * 2 * sizeof(float));
    p.keys_a = p.scores + up16(nq * rows * sizeof(float));
    const size_t n1 = rows > kSlice ? slices_of(rows) * k : 0;
    const size_t n2 = n1 > kSlice ? slices_of(n1) * k : 0;
    p.keys_b = p.keys_a + nq * n1 * sizeof(uint64_t);
    p.total = p.keys_b + nq * n2 * sizeof(uint64_t);
    return p;
}

template <int TQ>
void launch_scan(bool aligned, dim3 grid, hipStream_t st, const float *Q, const uint8_t *codes, const float *table,
                 const float *qstat, size_t rows, size_t dim, size_t j0, float *scores) {
    if (aligned)
        search_scan_kernel<TQ, true><<<grid, kScanThreads, 0, st>>>(Q, codes, table, qstat, rows, dim, j0, scores);
    else
        search_scan_kernel<TQ, false><<<grid, kScanThreads, 0, st>>>(Q, codes, table, qstat, rows, dim, j0, scores);
}

}  // namespace

SelectPlan select_plan(size_t nq, size_t rows, size_t k) {
    const SearchPlan p = search_plan(nq, rows, k);
    SelectPlan s;
    s.keys_a = p.keys_b - p.keys_a;
    s.keys_b = p.total - p.keys_b;
    return s;
}

bool select_grid_ok(size_t nq, size_t rows) { return rows == 0 || nq <= 0x7fffffffu / slices_of(rows); }

int select_topk(const float *sc, size_t nq, size_t rows, size_t k, uint64_t *keys_a, uint64_t *keys_b, int32_t *idx,
                float *scores, bool drop_nan, hipStream_t st) {
    uint64_t *keys[2] = {keys_a, keys_b};
    size_t n = rows;
    int pass = 0;
    for (;; ++pass) {
        const size_t nsl = slices_of(n);
        const int final = nsl == 1;
        const unsigned grid = static_cast<unsigned>(nq * nsl);
        uint64_t *dst = keys[pass & 1];
        if (pass == 0 && drop_nan)
            search_select_kernel<true, true><<<grid, kSelThreads, 0, st>>>(sc, nullptr, n, nsl, rows, static_cast<unsigned>(k),
                                                                           dst, idx, scores, final);
        else if (pass == 0)
            search_select_kernel<true><<<grid, kSelThreads, 0, st>>>(sc, nullptr, n, nsl, rows, static_cast<unsigned>(k),
                                                                     dst, idx, scores, final);
        else
            search_select_kernel<false><<<grid, kSelThreads, 0, st>>>(sc, keys[(pass - 1) & 1], n, nsl, rows,
                                                                      static_cast<unsigned>(k), dst, idx, scores, final);
        DLLM_LAUNCH_CHECK();
        if (final) break;
        n = nsl * k;
    }
    return DLLM_OK;
}

int select_fill_empty(size_t n, int32_t *idx, float *scores, hipStream_t st) {
    search_fill_empty_kernel<<<grid_for(n, 256, 0x7fffffffu), 256, 0, st>>>(n, idx, scores);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

}  // namespace dllm

using namespace dllm;

extern "C" {

size_t dllm_search_workspace(size_t nq, size_t rows, size_t k) { return search_plan(nq, rows, k).total; }

int dllm_search_table(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps,
                      float *table, dllm_stream_t stream) {
    if (int rc = search::check_store_shape(rows, dim)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!codes || !scales || !zps || !table) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    const int aligned = dim % 4 == 0 && reinterpret_cast<uintptr_t>(codes) % 4 == 0;
    const unsigned grid = static_cast<unsigned>((rows + kScanWaves * kTableRows - 1) / (kScanWaves * kTableRows));
    search_table_kernel<<<grid, kScanThreads, 0, as_stream(stream)>>>(codes, rows, dim, scales, zps, aligned, table);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

int dllm_search_vectors(const float *Q, size_t nq, const uint8_t *codes, const float *table, size_t rows, size_t dim,
                        size_t k, int32_t *idx, float *scores, void *workspace, size_t workspace_bytes,
                        dllm_stream_t stream) {
    if (int rc = search::check_k(k)) return rc;
    if (int rc = search::check_store_shape(rows, dim)) return rc;
    if (nq == 0) return DLLM_OK;
    if (!Q || !idx || !scores || (rows && (!codes || !table))) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    hipStream_t st = as_stream(stream);
    if (rows == 0) {
        search_fill_empty_kernel<<<grid_for(nq * k, 256, 0x7fffffffu), 256, 0, st>>>(nq * k, idx, scores);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    const SearchPlan plan = search_plan(nq, rows, k);
    if (!workspace || workspace_bytes < plan.total)
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace smaller than dllm_search_workspace(nq, rows, k)");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(DLLM_ERR_INVALID_PARAMS, "workspace must be 16-byte aligned");
    if (nq > 0x7fffffffu / slices_of(rows)) return fail(DLLM_ERR_SHAPE_MISMATCH, "nq * ceil(rows / 2048) exceeds the grid limit");
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    float *qstat = reinterpret_cast<float *>(ws + plan.qstat);
    float *sc = reinterpret_cast<float *>(ws + plan.scores);
    uint64_t *keys[2] = {reinterpret_cast<uint64_t *>(ws + plan.keys_a), reinterpret_cast<uint64_t *>(ws + plan.keys_b)};

    search_query_kernel<<<static_cast<unsigned>(nq), kStrands, 0, st>>>(Q, dim, qstat);
    DLLM_LAUNCH_CHECK();

    const bool aligned = dim % 4 == 0 && reinterpret_cast<uintptr_t>(codes) % 4 == 0 && reinterpret_cast<uintptr_t>(Q) % 16 == 0;
    const unsigned gx = static_cast<unsigned>((rows + kScanWaves * kScanRows - 1) / (kScanWaves * kScanRows));
    size_t j0 = 0;
    for (size_t tiles = nq / kScanTile; tiles; ) {   // grid.y holds at most 65535 tiles
        const unsigned gy = static_cast<unsigned>(tiles < 65535 ? tiles : 65535);
        launch_scan<kScanTile>(aligned, dim3(gx, gy), st, Q, codes, table, qstat, rows, dim, j0, sc);
        j0 += static_cast<size_t>(gy) * kScanTile;
        tiles -= gy;
    }
    if ((nq - j0) & 2) {
        launch_scan<2>(aligned, dim3(gx, 1), st, Q, codes, table, qstat, rows, dim, j0, sc);
        j0 += 2;
    }
    if ((nq - j0) & 1) launch_scan<1>(aligned, dim3(gx, 1), st, Q, codes, table, qstat, rows, dim, j0, sc);
    DLLM_LAUNCH_CHECK();

    if (int rc = select_topk(sc, nq, rows, k, keys[0], keys[1], idx, scores, false, st)) return rc;
    return DLLM_OK;
}

}  // extern "C"
