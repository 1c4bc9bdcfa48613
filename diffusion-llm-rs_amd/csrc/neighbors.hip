// neighbors.hip -- exact cosine k-NN between stored rows of the CompressedVector store: both sides of
// the product are byte codes, so the dot product is an integer and comes off the int8 matrix cores
// (v_mfma_i32_16x16x64_i8) exactly.  NsRouter::build_graph / build_edges (ns-router-rs/src/lib.rs:99-133)
// is the consumer.
//
// The rule (pair table, score, drops, key order) is pinned in include/dllm_quant.h 8l and its
// arithmetic lives in neighbor_rule.hpp; host_rules.cpp's dllm_neighbor_*_host is the plain C++ mirror
// and tests/neighbors_ref.py the numpy restatement.  All on the caller's stream, no atomics, no
// allocation:
//   neighbor_table_kernel  a wave per kTableRows rows: C1, C2 (exact u32), the f64 norm, (a, b, C1)
//   neighbor_scan_kernel   the hot path.  A workgroup of 4 waves owns kTileQ x kTileT = 64 query rows
//                          x 64 store rows, a wave 32 x 32 of it as 2 x 2 MFMA tiles of 16 x 16.  Per
//                          step of kStep = 64 bytes of the rows a lane loads 16 contiguous bytes of
//                          one row per fragment (both operands have k contiguous: no transpose, no
//                          LDS), flips bit 7 of every byte (c - 128 as an i8) and issues 4 MFMAs.
//                          The epilogue recovers D, applies the rule in f64 per accumulator element
//                          and writes f32 scores [nq][rows], a dropped pair as the NaN sentinel.
//   select                 search.hip's passes (search_select.hpp) with "NaN = no row".
#include "common.hpp"
#include "neighbor_rule.hpp"
#include "search_select.hpp"

#include <cmath>

namespace dllm {
namespace {

using neighbor::Entry;

constexpr int kWaveLanes = 64;
constexpr int kTableRows = 8;             // rows a table wave sums per pass
constexpr int kTableWaves = 4;
constexpr int kStep = 64;                 // bytes of a row one MFMA consumes (its K)
constexpr int kFrag = 16;                 // bytes of one row a lane holds per MFMA
constexpr int kMfma = 16;                 // rows / columns of one MFMA tile
constexpr int kWaveTiles = 2;             // MFMA tiles per wave, each way
constexpr int kWaveSide = kMfma * kWaveTiles;   // 32
constexpr int kBlockWaves = 2;            // waves per workgroup, each way
constexpr int kTileQ = kWaveSide * kBlockWaves; // 64 query rows per workgroup
constexpr int kTileT = kWaveSide * kBlockWaves; // 64 store rows per workgroup
constexpr int kScanThreads = kBlockWaves * kBlockWaves * kWaveLanes;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- pair table ------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kTableWaves * kWaveLanes) neighbor_table_kernel(const uint8_t *__restrict__ codes,
                                                                                 size_t rows, size_t dim,
                                                                                 const float *__restrict__ scales,
                                                                                 const float *__restrict__ zps,
                                                                                 int aligned, Entry *__restrict__ table) {
    const int lane = threadIdx.x & 63;
    const size_t row0 = (static_cast<size_t>(blockIdx.x) * kTableWaves + (threadIdx.x >> 6)) * kTableRows;
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
    if (aligned) {                             // dim % 4 == 0 and codes 4-byte aligned: a dword is all inside
        for (size_t d = 4 * static_cast<size_t>(lane); d < dim; d += 4 * kWaveLanes) {
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
        for (size_t d = lane; d < dim; d += kWaveLanes) {
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
        if (lane == r && row < rows)
            table[row] = neighbor::make_entry(scales[row], zps[row], c1[r], c2[r], static_cast<uint32_t>(dim));
    }
}

// ---- scan ------------------------------------------------------------------------------------------

// The lane's 16 bytes [off, off + 16) of the row at p, bit 7 of every byte flipped (c ^ 0x80 is
// c - 128 as an i8).  GUARD: the row's last, ragged step; a byte at d >= dim is never read and enters
// as 0x80, i.e. i8 zero after the flip.  VEC: 16 = dim % 16 == 0 and codes 16-byte aligned (one
// 16-byte load, wholly inside or outside the row), 4 = dim % 4 == 0 and codes 4-byte aligned (dwords
// likewise), 1 = bytes.
template <int VEC, bool GUARD>
__device__ __forceinline__ i32x4 load_frag(const uint8_t *__restrict__ p, size_t off, size_t dim) {
    uint32_t w[4];
    if (VEC == 16) {
        if (!GUARD || off < dim) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p + off);
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        } else {
            w[0] = w[1] = w[2] = w[3] = 0x80808080u;
        }
    } else if (VEC == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = (!GUARD || off + 4 * i < dim) ? *reinterpret_cast<const uint32_t *>(p + off + 4 * i) : 0x80808080u;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const size_t d = off + 4 * i + b;
                const uint32_t c = (!GUARD || d < dim) ? p[d] : 0x80u;
                w[i] |= c << (8 * b);
            }
        }
    }
    i32x4 f;
    f.x = static_cast<int>(w[0] ^ 0x80808080u);
    f.y = static_cast<int>(w[1] ^ 0x80808080u);
    f.z = static_cast<int>(w[2] ^ 0x80808080u);
    f.w = static_cast<int>(w[3] ^ 0x80808080u);
    return f;
}

template <int VEC, bool GUARD>
__device__ __forceinline__ void scan_step(const uint8_t *(&qp)[kWaveTiles], const uint8_t *(&tp)[kWaveTiles], size_t off,
                                          size_t dim, i32x4 (&acc)[kWaveTiles][kWaveTiles]) {
    i32x4 a[kWaveTiles], b[kWaveTiles];
#pragma unroll
    for (int m = 0; m < kWaveTiles; ++m) a[m] = load_frag<VEC, GUARD>(qp[m], off, dim);
#pragma unroll
    for (int n = 0; n < kWaveTiles; ++n) b[n] = load_frag<VEC, GUARD>(tp[n], off, dim);
#pragma unroll
    for (int m = 0; m < kWaveTiles; ++m)
#pragma unroll
        for (int n = 0; n < kWaveTiles; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b[n], acc[m][n], 0, 0, 0);
}

// grid.x: tiles of kTileT store rows; grid.y: tiles of kTileQ query rows from query j0 on.
// MFMA operands: A = query rows (lane l holds row l & 15, bytes 16 (l >> 4) .. + 15 of the step), B =
// store rows (the same map), so both fragments are 16 contiguous bytes of a row and the k order
// inside the instruction, whatever it is, is the same on both sides.  C: column (store row) l & 15,
// row (query) 4 (l >> 4) + register.
template <int VEC>
__global__ void __launch_bounds__(kScanThreads) neighbor_scan_kernel(const uint8_t *__restrict__ qcodes,
                                                                     const Entry *__restrict__ qtable, size_t nq,
                                                                     const uint8_t *__restrict__ codes,
                                                                     const Entry *__restrict__ table, size_t rows,
                                                                     size_t dim, float threshold, int64_t self_base,
                                                                     size_t j0, float *__restrict__ scores) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const size_t q0 = j0 + static_cast<size_t>(blockIdx.y) * kTileQ + static_cast<size_t>(wave / kBlockWaves) * kWaveSide;
    const size_t t0 = static_cast<size_t>(blockIdx.x) * kTileT + static_cast<size_t>(wave % kBlockWaves) * kWaveSide;
    if (q0 >= nq || t0 >= rows) return;
    const uint8_t *qp[kWaveTiles], *tp[kWaveTiles];
#pragma unroll
    for (int m = 0; m < kWaveTiles; ++m) {   // rows past the end re-read the last row; never stored
        const size_t q = q0 + m * kMfma + lr, t = t0 + m * kMfma + lr;
        qp[m] = qcodes + (q < nq ? q : nq - 1) * dim;
        tp[m] = codes + (t < rows ? t : rows - 1) * dim;
    }
    i32x4 acc[kWaveTiles][kWaveTiles];
#pragma unroll
    for (int m = 0; m < kWaveTiles; ++m)
#pragma unroll
        for (int n = 0; n < kWaveTiles; ++n) acc[m][n] = i32x4{0, 0, 0, 0};

    const size_t full = dim / kStep * kStep;
    size_t off = static_cast<size_t>(kFrag) * lg;
    for (; off < full; off += kStep) scan_step<VEC, false>(qp, tp, off, dim, acc);
    if (full < dim) scan_step<VEC, true>(qp, tp, off, dim, acc);

    const uint32_t udim = static_cast<uint32_t>(dim);
    Entry et[kWaveTiles];
    size_t tcol[kWaveTiles];
#pragma unroll
    for (int n = 0; n < kWaveTiles; ++n) {
        tcol[n] = t0 + n * kMfma + lr;
        et[n] = table[tcol[n] < rows ? tcol[n] : rows - 1];
    }
#pragma unroll
    for (int m = 0; m < kWaveTiles; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t q = q0 + m * kMfma + 4 * lg + i;
            if (q >= nq) continue;
            const Entry eq = qtable[q];
#pragma unroll
            for (int n = 0; n < kWaveTiles; ++n) {
                if (tcol[n] >= rows) continue;
                const uint32_t D = neighbor::dot_from_signed(acc[m][n][i], eq.c1, et[n].c1, udim);
                const float s = neighbor::score(eq.a, eq.b, eq.c1, et[n].a, et[n].b, et[n].c1, D, udim);
                const bool drop = neighbor::dropped(s, threshold, self_base, q, tcol[n]);
                scores[q * rows + tcol[n]] = drop ? __uint_as_float(0x7fc00000u) : s;
            }
        }
}

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// Workspace: scores f32 [nq][rows] | keys A | keys B (the select passes' candidate keys).
struct NeighborPlan {
    size_t keys_a = 0, keys_b = 0, total = 0;
};
NeighborPlan neighbor_plan(size_t nq, size_t rows, size_t k) {
    const SelectPlan s = select_plan(nq, rows, k);
    NeighborPlan p;
    p.keys_a = up16(nq * rows * sizeof(float));
    p.keys_b = p.keys_a + s.keys_a;
    p.total = p.keys_b + s.keys_b;
    return p;
}

template <int VEC>
void launch_scan(dim3 grid, hipStream_t st, const uint8_t *qcodes, const Entry *qtable, size_t nq, const uint8_t *codes,
                 const Entry *table, size_t rows, size_t dim, float threshold, int64_t self_base, size_t j0, float *sc) {
    neighbor_scan_kernel<VEC><<<grid, kScanThreads, 0, st>>>(qcodes, qtable, nq, codes, table, rows, dim, threshold,
                                                             self_base, j0, sc);
}

}  // namespace
}  // namespace dllm

using namespace dllm;

extern "C" {

size_t dllm_neighbor_workspace(size_t nq, size_t rows, size_t k) { return neighbor_plan(nq, rows, k).total; }

int dllm_neighbor_table(const uint8_t *codes, size_t rows, size_t dim, const float *scales, const float *zps, void *table,
                        dllm_stream_t stream) {
    if (int rc = search::check_store_shape(rows, dim)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!codes || !scales || !zps || !table) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (int rc = neighbor::check_table_aligned(table)) return rc;
    const int aligned = dim % 4 == 0 && reinterpret_cast<uintptr_t>(codes) % 4 == 0;
    const unsigned grid = static_cast<unsigned>((rows + kTableWaves * kTableRows - 1) / (kTableWaves * kTableRows));
    neighbor_table_kernel<<<grid, kTableWaves * kWaveLanes, 0, as_stream(stream)>>>(codes, rows, dim, scales, zps, aligned,
                                                                                    static_cast<Entry *>(table));
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

int dllm_neighbor_rows(const uint8_t *qcodes, const void *qtable, size_t nq, const uint8_t *codes, const void *table,
                       size_t rows, size_t dim, size_t k, float threshold, int64_t self_base, int32_t *idx, float *scores,
                       void *workspace, size_t workspace_bytes, dllm_stream_t stream) {
    if (int rc = neighbor::check_rows_args(nq, rows, dim, k, threshold, self_base)) return rc;
    if (nq == 0) return DLLM_OK;
    if (int rc = neighbor::check_rows_buffers(qcodes, qtable, codes, table, rows, idx, scores)) return rc;
    hipStream_t st = as_stream(stream);
    if (rows == 0) return select_fill_empty(nq * k, idx, scores, st);
    const NeighborPlan plan = neighbor_plan(nq, rows, k);
    if (!workspace || workspace_bytes < plan.total)
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace smaller than dllm_neighbor_workspace(nq, rows, k)");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(DLLM_ERR_INVALID_PARAMS, "workspace must be 16-byte aligned");
    if (!select_grid_ok(nq, rows)) return fail(DLLM_ERR_SHAPE_MISMATCH, "nq * ceil(rows / 2048) exceeds the grid limit");
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    float *sc = reinterpret_cast<float *>(ws);
    const Entry *qt = static_cast<const Entry *>(qtable), *tt = static_cast<const Entry *>(table);

    const uintptr_t both = reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(qcodes);
    const int vec = (dim % 16 == 0 && both % 16 == 0) ? 16 : (dim % 4 == 0 && both % 4 == 0) ? 4 : 1;
    const unsigned gx = static_cast<unsigned>((rows + kTileT - 1) / kTileT);
    size_t j0 = 0;
    for (size_t tiles = (nq + kTileQ - 1) / kTileQ; tiles; ) {   // grid.y holds at most 65535 tiles
        const unsigned gy = static_cast<unsigned>(tiles < 65535 ? tiles : 65535);
        const dim3 grid(gx, gy);
        if (vec == 16)
            launch_scan<16>(grid, st, qcodes, qt, nq, codes, tt, rows, dim, threshold, self_base, j0, sc);
        else if (vec == 4)
            launch_scan<4>(grid, st, qcodes, qt, nq, codes, tt, rows, dim, threshold, self_base, j0, sc);
        else
            launch_scan<1>(grid, st, qcodes, qt, nq, codes, tt, rows, dim, threshold, self_base, j0, sc);
        DLLM_LAUNCH_CHECK();
        j0 += static_cast<size_t>(gy) * kTileQ;
        tiles -= gy;
    }
    return select_topk(sc, nq, rows, k, reinterpret_cast<uint64_t *>(ws + plan.keys_a),
                       reinterpret_cast<uint64_t *>(ws + plan.keys_b), idx, scores, true, st);
}

}  // extern "C"
