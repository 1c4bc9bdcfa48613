// dedup.hip -- deduplication of the CompressedVector store on the device: hash every row's codes,
// keep the first row of each hash (in this batch or any earlier one on the same seen-set), copy the
// kept rows together.  The write path between dllm_compress_vectors and the search scan.
//
// The three rules (hash, filter, merge) are pinned in include/dllm_quant.h, section 8i; this file is
// their device form, host_rules.cpp's dllm_*_host entries the serial C++ mirror and tests/dedup_ref.py
// two Python restatements.  Everything is integer arithmetic: all of them agree to the bit.
//   dedup_hash_kernel<G>   the hot path: one read of the codes.  G lanes (4, 16 or 64) share a row;
//                          a lane takes aligned 16-byte pieces, folds each to its base-31 value,
//                          chains its pieces by 31^(16 G), and the lanes' sums are weighted by
//                          31^(16 lane) and added over the group.
//   dedup_insert_kernel    a thread per row: claims the hash's key slot (64-bit compare-and-swap,
//                          empty -> h; linear probing) and lowers the slot's value to the row's
//                          sequence number (64-bit atomic min).  Touches the table with atomics only.
//   dedup_resolve_kernel   after the launch boundary: looks each row up; keep = (value == own sequence
//                          number), first = value; counts the kept rows of each block of 1024.
//   dedup_scan_kernel      one workgroup: exclusive scan of the block counts, n_kept, the set's count.
//   dedup_scatter_kernel   ranks the kept rows inside their block and writes their indices ascending,
//                          -1 from n_kept on.
//   dedup_gather_kernel    copies row kept_rows[i] to row i of the output for i < n_kept (read on the device).
// No thread waits on another thread's store; every probe loop is bounded by the slot count; no
// allocation; all launches on the caller's stream.
//
// Reference: io-dedup/src/lib.rs:119-212 (store_vectors: compute_hash, deduplicate, merge_requests).
#include "common.hpp"
#include "dedup_rule.hpp"

namespace dllm {
namespace {

using namespace dedup;
typedef unsigned long long ull;

constexpr int kThreads = 256;
constexpr int kRowsPerThread = 4;
constexpr int kBlockRows = kThreads * kRowsPerThread;   // rows per resolve / scatter workgroup
constexpr int kScanThreads = 1024;

// ---- rule 1: the hash ------------------------------------------------------------------------------

// 31^(unit * e) for e < 2^BITS, by squaring: the factors 31^(unit 2^b) are compile-time constants.
template <int BITS>
__device__ __forceinline__ uint64_t pow_of(uint64_t base, unsigned e) {
    uint64_t r = 1;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        if ((e >> b) & 1u) r *= base;
        base *= base;
    }
    return r;
}

// 31^(-z) mod 2^64, z < 16.
struct InvPowTable {
    uint64_t v[16];
    constexpr InvPowTable() : v{} {
        uint64_t x = 1;
        for (int i = 0; i < 16; ++i) {
            v[i] = x;
            x *= inv31();
        }
    }
};
__constant__ const InvPowTable kInvPow = InvPowTable();

// The base-31 value of a dword's four codes, the byte at the lowest address the most significant
// digit: 31^3 b0 + 31^2 b1 + 31 b2 + b3 < 2^23.  Two byte dot products (weights 31, 1) and a multiply-add.
__device__ __forceinline__ uint32_t dword_value(uint32_t x) {
    const uint32_t hi = __builtin_amdgcn_udot4(x, 0x0000011fu, 0u, false);   // 31 b0 + b1
    const uint32_t lo = __builtin_amdgcn_udot4(x, 0x011f0000u, 0u, false);   // 31 b2 + b3
    return hi * 961u + lo;
}

// The base-31 value of 16 bytes: sum_i b_i 31^(15 - i) mod 2^64.
__device__ __forceinline__ uint64_t piece_value(const uint32_t (&w)[4]) {
    constexpr uint64_t kDword = pow31(4), kTwo = pow31(8);
    const uint64_t hi = dword_value(w[0]) * kDword + dword_value(w[1]);   // < 2^44: no wrap
    const uint64_t lo = dword_value(w[2]) * kDword + dword_value(w[3]);
    return hi * kTwo + lo;
}

// Zeroes the first `front` and the last `back` bytes of a piece (either may be 0; front + back < 16):
// the piece as two u64 halves, a 64-bit shift each.
__device__ __forceinline__ void mask_piece(uint32_t (&w)[4], unsigned front, unsigned back) {
    const uint64_t ones = ~uint64_t(0);
    const uint64_t lo = (front >= 8 ? 0 : ones << (8 * front)) & (back <= 8 ? ones : ones >> (8 * (back - 8)));
    const uint64_t hi = (front <= 8 ? ones : ones << (8 * (front - 8))) & (back >= 8 ? 0 : ones >> (8 * back));
    w[0] &= static_cast<uint32_t>(lo), w[1] &= static_cast<uint32_t>(lo >> 32);
    w[2] &= static_cast<uint32_t>(hi), w[3] &= static_cast<uint32_t>(hi >> 32);
}

// A piece at the buffer's edge, byte by byte: the bytes of the row only (an index outside the row
// re-reads the row's nearest byte; mask_piece drops it).  Two pieces of a whole call come here, so
// the loop is left rolled.
__device__ __forceinline__ void edge_piece(const uint8_t *row, int at, int dim, uint32_t (&w)[4]) {
    uint64_t lo = 0, hi = 0;
#pragma unroll 1
    for (int i = 0; i < 16; ++i) {
        int idx = at + i;
        idx = idx < 0 ? 0 : (idx >= dim ? dim - 1 : idx);
        const uint64_t b = row[idx];
        if (i < 8) lo |= b << (8 * i);
        else hi |= b << (8 * (i - 8));
    }
    w[0] = static_cast<uint32_t>(lo), w[1] = static_cast<uint32_t>(lo >> 32);
    w[2] = static_cast<uint32_t>(hi), w[3] = static_cast<uint32_t>(hi >> 32);
}

// Four sums over the G lanes of a group at once: the first two levels hand half of the sums to the
// partner lane and add the partner's half of the others (2 + 1 shuffles instead of 4 + 4), the rest
// is a plain butterfly.  Every lane ends with the whole-group sum number 2 [sub & G/2] + [sub & G/4].
template <int G>
__device__ __forceinline__ uint64_t group_sum4(const uint64_t (&a)[4], int sub) {
    const bool up1 = (sub & (G / 2)) != 0, up2 = (sub & (G / 4)) != 0;
    const uint64_t k0 = up1 ? a[2] : a[0], k1 = up1 ? a[3] : a[1], s0 = up1 ? a[0] : a[2], s1 = up1 ? a[1] : a[3];
    const uint64_t b0 = k0 + static_cast<uint64_t>(__shfl_xor(static_cast<ull>(s0), G / 2, 64));
    const uint64_t b1 = k1 + static_cast<uint64_t>(__shfl_xor(static_cast<ull>(s1), G / 2, 64));
    uint64_t c = (up2 ? b1 : b0) + static_cast<uint64_t>(__shfl_xor(static_cast<ull>(up2 ? b0 : b1), G / 4, 64));
#pragma unroll
    for (int m = G / 8; m > 0; m >>= 1) c += static_cast<uint64_t>(__shfl_xor(static_cast<ull>(c), m, 64));
    return c;
}

// A row is cut into 16-byte pieces at the 16-byte boundaries of memory, not of the row: with o = the
// row's first address mod 16 there are n = ceil((o + dim) / 16) pieces, the first with o bytes in
// front of the row and the last with z = 16 n - (o + dim) bytes behind it, both counted as zero
// digits.  Every piece is one aligned 16-byte load, the bytes outside the row masked off; the two
// pieces that would leave the buffer [codes, codes + (rows - 1) ld + dim) -- the first row's front
// and the last row's back -- are read byte by byte instead, so nothing outside the buffer is touched.
// Pieces are numbered from the row's end, k = 0 the last; lane s of the group takes k = s, s + G, ...
// and chains them from the highest k down: acc = acc 31^(16 G) + value.  Piece k's lowest digit has
// weight 31^(16 k - z), so
//   h = 31^(-z) sum_s 31^(16 s) acc_s     (31 is odd: 31^(-1) exists mod 2^64; the z zero digits
// behind the row made the sum an exact multiple of 31^z).
// (A buffer of under 31 bytes may hold no whole aligned piece; dedup_hash_tiny_kernel folds it serially.)
// A group keeps kHashRows rows in flight: their loads are issued together, and one reduction sums all four.
constexpr int kHashRows = 4;
// Group width by row length, so that a lane chains several pieces and the per-row set-up and
// reduction are shared by more rows of a wave: 4 lanes up to 256 codes (64 rows a wave), 16 lanes up
// to 2048 (16 rows a wave), a whole wave beyond (4 rows).  At 1 Mi x 768 one wave a row ran at 3.15
// TB/s and 16 lanes a row at 4.99.
constexpr size_t kShortDim = 256, kMidDim = 2048;

template <int G>
__global__ void __launch_bounds__(kThreads) dedup_hash_kernel(const uint8_t *__restrict__ codes, size_t rows, size_t dim,
                                                              size_t ld, uint64_t *__restrict__ hashes) {
    constexpr int kGroups = 64 / G, R = kHashRows;
    constexpr int kLog = G == 4 ? 2 : (G == 16 ? 4 : 6);
    constexpr uint64_t kPiece = pow31(16), kTrip = pow31(16 * G);
    const int lane = threadIdx.x & 63, sub = lane % G;
    const size_t wave = static_cast<size_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave * (kGroups * R) >= rows) return;
    const size_t row0 = (wave * kGroups + lane / G) * R;
    const uint8_t *buf_end = codes + (rows - 1) * ld + dim;
    const uint8_t *safe = codes + ((16u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(codes) & 15u)) & 15u);   // a whole piece: the buffer has >= 31 bytes
    const unsigned trips = ((static_cast<unsigned>(dim) + 30u) / 16u + G - 1) / G;   // n <= (15 + dim + 15) / 16

    const uint8_t *a0[R];
    unsigned o[R], n[R], z[R];
    uint64_t acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {   // a group's rows past the end re-read the last row; never stored
        const uint8_t *p = codes + (row0 + r < rows ? row0 + r : rows - 1) * ld;
        o[r] = static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) & 15u);
        a0[r] = p - o[r];
        const unsigned span = o[r] + static_cast<unsigned>(dim);
        n[r] = (span + 15u) >> 4;
        z[r] = 16u * n[r] - span;
        acc[r] = 0;
    }
    for (unsigned t = trips; t-- > 0;) {
        const unsigned k = sub + t * G;
        uint32_t w[R][4];
        unsigned j[R];
        bool inside[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {                       // the loads of all the rows first: they overlap
            const unsigned kc = k < n[r] ? k : n[r] - 1;   // a lane with no piece this trip re-reads the row's first; dropped below
            j[r] = n[r] - 1 - kc;
            const uint8_t *c = a0[r] + 16u * static_cast<size_t>(j[r]);
            inside[r] = c >= codes && c + 16 <= buf_end;
            const uint4 v = *reinterpret_cast<const uint4 *>(inside[r] ? c : safe);   // unconditional: nothing waits here
            w[r][0] = v.x, w[r][1] = v.y, w[r][2] = v.z, w[r][3] = v.w;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!inside[r])                                 // the buffer's first or last piece
                edge_piece(a0[r] + o[r], static_cast<int>(16u * j[r]) - static_cast<int>(o[r]), static_cast<int>(dim), w[r]);
            const unsigned front = j[r] == 0 ? o[r] : 0u, back = j[r] == n[r] - 1 ? z[r] : 0u;
            if (front | back) mask_piece(w[r], front, back);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = acc[r] * kTrip + (k < n[r] ? piece_value(w[r]) : uint64_t(0));
    }
    const uint64_t weight = pow_of<kLog>(kPiece, static_cast<unsigned>(sub));
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] *= weight;
    const uint64_t sum = group_sum4<G>(acc, sub);
    const size_t row = row0 + ((sub & (G / 2)) ? 2 : 0) + ((sub & (G / 4)) ? 1 : 0);
    if ((sub & (G / 4 - 1)) == 0 && row < rows) {
        const unsigned span = static_cast<unsigned>(reinterpret_cast<uintptr_t>(codes + row * ld) & 15u) + static_cast<unsigned>(dim);
        hashes[row] = sum * kInvPow.v[(16u - (span & 15u)) & 15u];
    }
}

// The whole buffer is under 31 bytes: a thread per row, the reference's fold.
__global__ void dedup_hash_tiny_kernel(const uint8_t *__restrict__ codes, size_t rows, size_t dim, size_t ld,
                                       uint64_t *__restrict__ hashes) {
    const size_t r = threadIdx.x;
    if (r >= rows) return;
    uint64_t acc = 0;
    for (size_t i = 0; i < dim; ++i) acc = acc * 31u + codes[r * ld + i];
    hashes[r] = acc;
}

// ---- rule 2: the filter ----------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) dedup_init_kernel(uint64_t *__restrict__ tab, size_t words) {
    const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < words; i += stride)
        tab[i] = (i == kFlagWord || i == kCountWord || i == 3) ? 0 : ~uint64_t(0);
}

__global__ void __launch_bounds__(kThreads) dedup_insert_kernel(const uint64_t *__restrict__ hashes, size_t rows,
                                                                uint64_t base, uint64_t *tab, size_t slots) {
    const size_t r = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
    const ull h = r < rows ? hashes[r] : 0ull, seq = base + r;
    // A row whose left neighbour in the wave has the same hash leaves the table to it: the neighbour's
    // sequence number is smaller, so this row's atomic min could not change the value.  Runs of equal
    // rows (an all-zero prefill, padding) then cost one pair of atomics per wave, not one per row.
    const ull left = __shfl_up(h, 1, 64);
    if (r >= rows || ((threadIdx.x & 63) != 0 && left == h)) return;
    ull *t = reinterpret_cast<ull *>(tab);
    if (h == kEmptyKey) {
        atomicMin(t + kSideWord, seq);
        return;
    }
    ull *keys = t + kHeaderWords, *vals = keys + slots;
    const size_t mask = slots - 1;
    size_t s = first_slot(h, mask);
    for (size_t probe = 0; probe < slots; ++probe) {
        const ull old = atomicCAS(keys + s, static_cast<ull>(kEmptyKey), h);
        if (old == kEmptyKey || old == h) {
            atomicMin(vals + s, seq);
            return;
        }
        s = (s + 1) & mask;
    }
    atomicCAS(t + kFlagWord, 0ull, 1ull);   // the table is full: this row will be looked up and not found
}

// Sum of x over the workgroup's threads before this one, and (to every thread) the total.
template <int THREADS>
__device__ __forceinline__ unsigned block_exclusive(unsigned x, unsigned *lds, unsigned &total) {
    constexpr int kWaves = THREADS / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    __syncthreads();                      // the previous use of lds is over
    if (lane == 63) lds[wv] = incl;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        const unsigned v = lds[i];
        if (i < wv) before += v;
        total += v;
    }
    return before + incl - x;
}

__global__ void __launch_bounds__(kThreads) dedup_resolve_kernel(const uint64_t *__restrict__ hashes, size_t rows,
                                                                 uint64_t base, const uint64_t *__restrict__ tab,
                                                                 size_t slots, uint8_t *__restrict__ keep,
                                                                 uint64_t *__restrict__ first,
                                                                 uint32_t *__restrict__ counts) {
    __shared__ unsigned lds[kThreads / 64];
    const uint64_t *keys = tab + kHeaderWords, *vals = keys + slots;
    const size_t mask = slots - 1;
    const size_t r0 = static_cast<size_t>(blockIdx.x) * kBlockRows + static_cast<size_t>(threadIdx.x) * kRowsPerThread;
    unsigned kept = 0;
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        const size_t r = r0 + i;
        if (r >= rows) break;
        const uint64_t h = hashes[r];
        uint64_t v = kNoSeq;
        if (h == kEmptyKey) {
            v = tab[kSideWord];
        } else {
            size_t s = first_slot(h, mask);
            for (size_t probe = 0; probe < slots; ++probe) {
                const uint64_t key = keys[s];
                if (key == h) {
                    v = vals[s];
                    break;
                }
                if (key == kEmptyKey) break;
                s = (s + 1) & mask;
            }
        }
        const bool k = v == base + r;
        keep[r] = k ? 1 : 0;
        first[r] = v;
        kept += k ? 1u : 0u;
    }
    unsigned total;
    block_exclusive<kThreads>(kept, lds, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[b] becomes the number of kept rows in blocks before b; one workgroup, chunks of kScanThreads.
__global__ void __launch_bounds__(kScanThreads) dedup_scan_kernel(uint32_t *__restrict__ counts, size_t nblocks,
                                                                  uint32_t *__restrict__ n_kept, uint64_t *tab) {
    __shared__ unsigned lds[kScanThreads / 64];
    unsigned carry = 0;
    for (size_t c0 = 0; c0 < nblocks; c0 += kScanThreads) {
        const size_t i = c0 + threadIdx.x;
        const unsigned x = i < nblocks ? counts[i] : 0u;
        unsigned total;
        const unsigned ex = block_exclusive<kScanThreads>(x, lds, total);
        if (i < nblocks) counts[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        *n_kept = carry;
        tab[kCountWord] += carry;   // every kept row is a hash the set had not held
    }
}

__global__ void __launch_bounds__(kThreads) dedup_scatter_kernel(const uint8_t *__restrict__ keep, size_t rows,
                                                                 const uint32_t *__restrict__ counts,
                                                                 const uint32_t *__restrict__ n_kept,
                                                                 int32_t *__restrict__ kept_rows) {
    __shared__ unsigned lds[kThreads / 64];
    const size_t r0 = static_cast<size_t>(blockIdx.x) * kBlockRows + static_cast<size_t>(threadIdx.x) * kRowsPerThread;
    bool k[kRowsPerThread];
    unsigned mine = 0;
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        k[i] = r0 + i < rows && keep[r0 + i] != 0;
        mine += k[i] ? 1u : 0u;
    }
    unsigned total;
    size_t at = static_cast<size_t>(counts[blockIdx.x]) + block_exclusive<kThreads>(mine, lds, total);
    const size_t n = *n_kept;
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        const size_t r = r0 + i;
        if (r >= rows) break;
        if (k[i]) kept_rows[at++] = static_cast<int32_t>(r);   // at < n: a kept row's rank
        if (r >= n) kept_rows[r] = -1;                         // the tail: never a rank
    }
}

// ---- rule 3: the merge -----------------------------------------------------------------------------

// A wave per kept row, round-robin.  VEC: dim, both strides and both base addresses are multiples of
// 16, so a row is whole 16-byte pieces; otherwise bytes.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) dedup_gather_kernel(const uint8_t *__restrict__ codes, size_t dim, size_t ld,
                                                                const int32_t *__restrict__ kept_rows,
                                                                const uint32_t *__restrict__ n_kept,
                                                                uint8_t *__restrict__ out, size_t out_ld) {
    const int lane = threadIdx.x & 63;
    const size_t n = *n_kept;
    const size_t waves = static_cast<size_t>(gridDim.x) * (kThreads / 64);
    for (size_t i = static_cast<size_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); i < n; i += waves) {
        const int32_t r = kept_rows[i];
        if (r < 0) continue;
        const uint8_t *src = codes + static_cast<size_t>(r) * ld;
        uint8_t *dst = out + i * out_ld;
        if (VEC) {
            for (size_t d = 16 * static_cast<size_t>(lane); d < dim; d += 16 * 64)
                *reinterpret_cast<uint4 *>(dst + d) = *reinterpret_cast<const uint4 *>(src + d);
        } else {
            for (size_t d = lane; d < dim; d += 64) dst[d] = src[d];
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
inline size_t blocks_of(size_t rows) { return (rows + kBlockRows - 1) / kBlockRows; }
// The slots of the one-shot filter's own table: a power of two >= 2 rows.
inline size_t oneshot_slots(size_t rows) {
    size_t s = 2;
    while (s < 2 * rows) s <<= 1;
    return s;
}

}  // namespace
}  // namespace dllm

using namespace dllm;

extern "C" {

int dllm_hash_rows(const uint8_t *codes, size_t rows, size_t dim, size_t ld, uint64_t *hashes, dllm_stream_t stream) {
    if (int rc = check_hash_args(rows, dim, ld)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!codes || !hashes) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(hashes) % 8) return fail(DLLM_ERR_INVALID_PARAMS, "hashes must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    const size_t waves_per_block = kThreads / 64;
    if ((rows - 1) * ld + dim < 31) {   // at most 30 rows
        dedup_hash_tiny_kernel<<<1, 64, 0, st>>>(codes, rows, dim, ld, hashes);
    } else if (dim <= kShortDim) {
        const size_t per = waves_per_block * (64 / 4) * kHashRows;
        dedup_hash_kernel<4><<<static_cast<unsigned>((rows + per - 1) / per), kThreads, 0, st>>>(codes, rows, dim, ld, hashes);
    } else if (dim <= kMidDim) {
        const size_t per = waves_per_block * (64 / 16) * kHashRows;
        dedup_hash_kernel<16><<<static_cast<unsigned>((rows + per - 1) / per), kThreads, 0, st>>>(codes, rows, dim, ld, hashes);
    } else {
        const size_t per = waves_per_block * kHashRows;
        dedup_hash_kernel<64><<<static_cast<unsigned>((rows + per - 1) / per), kThreads, 0, st>>>(codes, rows, dim, ld, hashes);
    }
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

int dllm_dedup_table_init(void *table, size_t slots, dllm_stream_t stream) {
    if (int rc = check_slots(slots)) return rc;
    if (!table) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (int rc = check_table_aligned(table)) return rc;
    const size_t words = table_words(slots);
    dedup_init_kernel<<<grid_for(words, kThreads), kThreads, 0, as_stream(stream)>>>(static_cast<uint64_t *>(table), words);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

size_t dllm_dedup_workspace(size_t rows) {
    if (rows >= kMaxRows) return 0;
    return up16(blocks_of(rows) * sizeof(uint32_t)) + dllm_dedup_table_bytes(oneshot_slots(rows));
}

int dllm_dedup_rows(const uint64_t *hashes, size_t rows, uint64_t base, void *table, size_t slots, uint8_t *keep,
                    uint64_t *first, int32_t *kept_rows, uint32_t *n_kept, void *workspace, size_t workspace_bytes,
                    dllm_stream_t stream) {
    if (int rc = check_filter_args(rows, base, table, slots)) return rc;
    if (rows == 0) return DLLM_OK;
    if (!hashes || !keep || !first || !kept_rows || !n_kept) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (!workspace || workspace_bytes < dllm_dedup_workspace(rows))
        return fail(DLLM_ERR_INVALID_PARAMS, "workspace smaller than dllm_dedup_workspace(rows)");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(DLLM_ERR_INVALID_PARAMS, "workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(hashes) % 8 || reinterpret_cast<uintptr_t>(first) % 8 ||
        reinterpret_cast<uintptr_t>(kept_rows) % 4 || reinterpret_cast<uintptr_t>(n_kept) % 4)
        return fail(DLLM_ERR_INVALID_PARAMS, "hashes and first must be 8-byte, kept_rows and n_kept 4-byte aligned");
    hipStream_t st = as_stream(stream);
    const size_t nblocks = blocks_of(rows);
    uint32_t *counts = static_cast<uint32_t *>(workspace);
    uint64_t *tab = static_cast<uint64_t *>(table);
    if (!tab) {   // the one-shot form: a table of its own in the workspace, empty at every call
        tab = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(workspace) + up16(nblocks * sizeof(uint32_t)));
        slots = oneshot_slots(rows);
        const size_t words = table_words(slots);
        dedup_init_kernel<<<grid_for(words, kThreads), kThreads, 0, st>>>(tab, words);
        DLLM_LAUNCH_CHECK();
    }
    dedup_insert_kernel<<<static_cast<unsigned>((rows + kThreads - 1) / kThreads), kThreads, 0, st>>>(hashes, rows, base, tab, slots);
    DLLM_LAUNCH_CHECK();
    dedup_resolve_kernel<<<static_cast<unsigned>(nblocks), kThreads, 0, st>>>(hashes, rows, base, tab, slots, keep, first, counts);
    DLLM_LAUNCH_CHECK();
    dedup_scan_kernel<<<1, kScanThreads, 0, st>>>(counts, nblocks, n_kept, tab);
    DLLM_LAUNCH_CHECK();
    dedup_scatter_kernel<<<static_cast<unsigned>(nblocks), kThreads, 0, st>>>(keep, rows, counts, n_kept, kept_rows);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

int dllm_gather_rows(const uint8_t *codes, size_t dim, size_t ld, const int32_t *kept_rows, const uint32_t *n_kept,
                     uint8_t *out, size_t out_ld, dllm_stream_t stream) {
    if (int rc = check_gather_args(dim, ld, out_ld)) return rc;
    if (!codes || !kept_rows || !n_kept || !out) return fail(DLLM_ERR_INVALID_PARAMS, "NULL argument");
    if (reinterpret_cast<uintptr_t>(kept_rows) % 4 || reinterpret_cast<uintptr_t>(n_kept) % 4)
        return fail(DLLM_ERR_INVALID_PARAMS, "kept_rows and n_kept must be 4-byte aligned");
    const bool vec = (dim | ld | out_ld | reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const unsigned grid = kCUs * 8;
    if (vec)
        dedup_gather_kernel<true><<<grid, kThreads, 0, as_stream(stream)>>>(codes, dim, ld, kept_rows, n_kept, out, out_ld);
    else
        dedup_gather_kernel<false><<<grid, kThreads, 0, as_stream(stream)>>>(codes, dim, ld, kept_rows, n_kept, out, out_ld);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

}  // extern "C"
