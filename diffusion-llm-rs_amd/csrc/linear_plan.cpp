// linear_plan.cpp -- the linear layer's kernel selection (see linear_plan.hpp).  The measured numbers
// and profiles/ citations beside each threshold are the record of why it stands where it does.
#include "linear_plan.hpp"

#include <algorithm>
#include <cstdlib>

namespace dllm {

PlanError check_shape(size_t K, size_t N, uint8_t bits, size_t group, int flags) {
    const int precision = flags & ~DLLM_LINEAR_PREFILL_ONLY;
    if (bits != 2 && bits != 4 && bits != 8) return {DLLM_ERR_UNSUPPORTED, "linear layer supports bits in {2, 4, 8}"};
    if (K == 0 || N == 0) return {DLLM_ERR_SHAPE_MISMATCH, "K and N must be >= 1"};
    if (K % kBK) return {DLLM_ERR_SHAPE_MISMATCH, "K must be a multiple of 64"};
    if (group == 0 || group % kBK) return {DLLM_ERR_INVALID_PARAMS, "group must be a positive multiple of 64"};
    if (K > (1u << 30) || N > (1u << 30)) return {DLLM_ERR_SHAPE_MISMATCH, "dimension too large"};
    if (precision != DLLM_PRECISION_EXACT && precision != DLLM_PRECISION_F16W)
        return {DLLM_ERR_INVALID_PARAMS, "precision must be DLLM_PRECISION_EXACT or DLLM_PRECISION_F16W"};
    return {};
}

PlanError check_plan_args(size_t N, size_t M, int fused) {
    if (M == 0 || M > (1u << 30)) return {DLLM_ERR_SHAPE_MISMATCH, "M must be 1..2^30"};
    if (fused && N % 4) return {DLLM_ERR_UNSUPPORTED, "fused p_sample needs N % 4 == 0"};
    return {};
}

PlanShape plan_shape_for(size_t K, size_t N, uint8_t bits, size_t group, int flags, int horner_ok) {
    PlanShape s;
    s.K = K; s.N = N; s.Npad = (N + kBN - 1) / kBN * kBN; s.group = group;
    s.bits = bits; s.precision = flags & ~DLLM_LINEAR_PREFILL_ONLY;
    s.decode_layout = (flags & DLLM_LINEAR_PREFILL_ONLY) == 0;
    // a handle's ratios exist (and can pass the check) only for the Horner-form shapes
    s.horner_ok = horner_ok != 0 && horner_shape(&s);
    return s;
}

bool exact_gemm_supported(int M, int K, int Npad, int group) {
    return M >= 1 && Npad % 128 == 0 && K % group == 0 && (group == 64 || group == 128 || group == 256);
}

// Exact-weight kernels apply when the group tiles K (a stage never straddles two groups).
bool use_exact(const PlanShape *h) {
    return h->precision == DLLM_PRECISION_EXACT &&
           exact_gemm_supported(1, static_cast<int>(h->K), static_cast<int>(h->Npad), static_cast<int>(h->group));
}

// ---- decode (M <= kDecodeMaxM, decode layout) --------------------------------------------------

size_t xl_lds_bytes(int M, int K, int group) {
    const size_t nq = static_cast<size_t>((K / group + 3) / 4);
    return static_cast<size_t>(M + 1) * (2 * static_cast<size_t>(K) + 16) + 2 * nq * 256;
}

namespace {
// Decode tile policy: (NT, nsplit) per M bucket, chosen from the M-sweep.
// Measured (scripts/decode_sweep.py, 48-layer graph, K = N = 4096 int4, us per layer;
// profiles/r01_decode_tiles): up to M = 32 the one-tile kernel wins (M 1/16/32: 5.1/6.9/10.7;
// the slab combine's extra launch costs ~4.7 us and NT = 4 without a split leaves 64 blocks whose
// per-CU load rate bounds the stream); at M 33..64 X re-reads dominate and NT 4 x 4 K-slices
// wins (M 64: 13.8 vs 18.6).
void decode_policy(int M, int &nt, int &nsplit) {
    nt = nsplit = M > 32 ? 4 : 1;
}
}  // namespace

// The decode plan for M <= kDecodeMaxM rows: tile_m = the M bucket (16 MT), tile_n = 16 NT, nsplit
// K slices of whole 128-deep slabs, DLLM_PLAN_DECODE_XL where X is staged in LDS.  nt0 / nsplit0 > 0:
// the lab build's (NT, nsplit) override in place of decode_policy.
void decode_plan(const PlanShape *h, int M, dllm_linear_plan_t *p, int nt0, int nsplit0) {
    int nt, nsplit;
    decode_policy(M, nt, nsplit);
    if (nt0 > 0) { nt = nt0; nsplit = nsplit0; }
    // the column group must tile Npad (a multiple of 128)
    while (nt > 1 && h->Npad % (16 * nt)) nt /= 2;
    const int K = static_cast<int>(h->K), gr = static_cast<int>(h->group);
    const int nslab = (K + 127) / 128;
    nsplit = std::max(1, std::min(nsplit, nslab));
    p->kernel = DLLM_KERNEL_DECODE;
    p->tile_m = M <= 16 ? 16 : (M <= 32 ? 32 : 64);
    p->tile_n = 16 * nt;
    p->kgroups = 1;
    p->nsplit = nsplit;
    p->flags = nsplit > 1 ? DLLM_PLAN_SPLITK : 0;
    // X and the scales staged in LDS (XL), M 9..16 only: M = 16 6.75 vs 7.25 us per layer in the
    // 40-layer chain, M = 1 / 2 / 4 / 8 5.16 / 5.34 / 5.58 / 6.00 vs 5.18 / 5.38 / 5.47 / 5.94
    // (profiles/r05_decode_xl/): fewer load instructions do not shorten the M <= 8 layer, whose
    // time is the weight stream's latency, and the DMA wait + barrier before the first MFMA costs a
    // little there.
    if (nsplit == 1 && nt == 1 && M <= 16 && use_exact(h) && gr != 64 && M > 8 && K % 512 == 0 &&
        nslab >= kDecWaves && xl_lds_bytes(M, K, gr) <= kXlLdsMax)
        p->flags |= DLLM_PLAN_DECODE_XL;
}

// ---- rounded weights (DLLM_PRECISION_F16W, or a group that does not tile K) ---------------------

// Rounded-weight (DLLM_PRECISION_F16W) tile policy: the largest tile that still gives >= 256
// blocks -- 256 x 256 (8 waves), 256 x 128 (8 waves, two k-groups) -- below that 128 x 128 tiles
// (two k-groups) with K split until ~200+ blocks (slab partials + ordered combine).
void rounded_plan(const PlanShape *h, int M, dllm_linear_plan_t *p) {
    const int np = static_cast<int>(h->Npad);
    const int mb256 = (M + 255) / 256, mb128 = (M + 127) / 128;
    auto set = [&](int tm, int tn, int kg, int ns) {
        p->kernel = DLLM_KERNEL_ROUNDED_RING;
        p->tile_m = tm; p->tile_n = tn; p->kgroups = kg; p->nsplit = ns;
        p->flags = ns > 1 ? DLLM_PLAN_SPLITK : 0;
    };
    if (np % 256 == 0 && mb256 * (np / 256) >= kCUs) return set(256, 256, 1, 1);
    if (mb256 * (np / 128) >= kCUs) return set(256, 128, 2, 1);
    const int tiles = mb128 * (np / 128);
    const int nk = static_cast<int>(h->K / kBK);
    int nsplit = 1;
    while (tiles * nsplit < 200 && nsplit < 8 && nk % (2 * nsplit) == 0 && nk / (2 * nsplit) >= 4) nsplit *= 2;
    return set(128, 128, 2, nsplit);
}

// ---- exact weights, Horner form ----------------------------------------------------------------

// Exact-weight GEMM in Horner form: for int4 g128 (and, on 256 x 256 tiles, int2 g128).  The ratios
// and their validity are decided once, by the handle's create (finish_linear); a handle whose
// scales fail the check runs the fold-form exact kernels.
#if DLLM_LAB
bool lab_horner128() {
    static const bool on = std::getenv("DLLM_LAB_HORNER128") != nullptr;
    return on;
}
#endif

// int4 and (256 x 256 tiles only: horner_ready) int2 codes, group 128.
bool horner_shape(const PlanShape *h) {
    return h->precision == DLLM_PRECISION_EXACT && (h->bits == 4 || h->bits == 2) && h->group == 128 &&
           h->K % 128 == 0 && h->Npad % 256 == 0;
}

namespace {

// The Horner kernel on 256 x 256 tiles (linear_horner.hip).  A grid short of a round takes the
// larger tiles when the alternative needs more rounds -- a 256 x 256 Horner round takes about two
// 128 x 256 PC rounds, a 128 x 256 PC round about 1.78 two-k-group 128 x 128 rounds (58.6 vs 33 us
// at K 4096).  Against the earlier full-round thresholds, N 4096, 40-layer chain
// (profiles/r06_tiles/policy_rounds_ab.jsonl): M 1100 / 1280 / 1536 / 1800: 63.2 / 61.0 / 62.1 /
// 68.2 -> 56.8 / 52.3 / 53.2 / 59.0 us (128 x 256 PC tiles short of a round), M 2304 / 2560 / 3072 /
// 3584: 106.5 / 106.7 / 107.7 / 112.6 -> 97.3 / 97.3 / 98.4 / 104.0 us (256 x 256 Horner tiles short
// of a round), M 2048 and 4096 unchanged.
bool horner_ready(const PlanShape *hc, int M) {
    const int np = static_cast<int>(hc->Npad);
    if (!horner_shape(hc)) return false;
    // rounds of 256 tiles: a 256 x 256 round takes about two 128 x 256 rounds, so the Horner grid
    // must not need more rounds than half the fold form's (M = 4300: 2 vs 3 rounds -> fold form)
    const int t256 = ((M + 255) / 256) * (np / 256), t128 = ((M + 127) / 128) * (np / 256);
#if DLLM_LAB
    if (hc->variant == 14) return false;   // lab A/B: the fold-form exact policy
    if (lab_horner128()) {                 // lab A/B: Horner form on 128 x 256 tiles
        if (t128 < kCUs) return false;
    } else
#endif
    if (2 * ((t256 + kCUs - 1) / kCUs) > (t128 + kCUs - 1) / kCUs)
        return false;
    // the handle's Horner ratios are valid (decided at create, immutable afterwards)
    return hc->horner_ok;
}

// The KG2 Horner kernel (256 x 128 tiles, two k-groups): where neither the 256 x 256 Horner grid
// nor the fold form's 128 x 256 grid fills a round but the 256 x 128 grid does (N = 4096: M
// 1793..1920; measured at M = 1800: 69.2 vs 74.9 us).  At M = 2048 the 128 x 256 fold grid fills
// the chip and is as fast (68.5 vs 69.6 us: KG2 stages two K-halves' X slices, 72 KiB per k-step
// against 24 KiB for the same MFMAs; profiles/r03_kg2/).  prefill_plan asks horner_pc_ready first,
// which by the rounds rule takes M 1793..1920 at N = 4096 (240 PC tiles against two rounds of
// 128 x 128): what reaches this kernel now is ceil(M / 128) == ceil(M / 256), i.e. M <= 128, on 256
// to 510 column tiles of 128 (M = 100, K = 512, N = 32768; tests/test_gpu_linear_kernels.py).
bool horner_kg2_ready(const PlanShape *hc, int M) {
    const int np = static_cast<int>(hc->Npad);
    if (!(hc->precision == DLLM_PRECISION_EXACT && hc->bits == 4 && hc->group == 128 && hc->K % 256 == 0 &&
          np % 128 == 0 && hc->horner_ok))
        return false;
#if DLLM_LAB
    if (hc->variant == 14 || hc->variant == 28) return false;   // lab A/B: the fold-form exact policy
#endif
    const int t256 = ((M + 255) / 256) * (np / 256), tk = ((M + 255) / 256) * (np / 128);
    const int t128 = ((M + 127) / 128) * (np / 256);
    return t256 < kCUs && t128 < kCUs && tk >= kCUs;
}

// The producer / consumer Horner kernel (128 x 256 tiles, linear_pc.hip): where the 256 x 256
// Horner grid does not fill a round and the 128 x 256 grid does (N = 4096: M 1921..4096 minus the
// Horner grid's own range; M = 2048 = config C2 and the C5 layers; the 2-GPU column shard), or,
// short of a round, where the two-k-group 128 x 128 grid would need 1.78x as many rounds or more.
bool horner_pc_ready(const PlanShape *hc, int M) {
    const int np = static_cast<int>(hc->Npad);
    if (hc->bits != 4 || !horner_shape(hc) || !hc->horner_ok) return false;
#if DLLM_LAB
    if (hc->variant == 14 || hc->variant == 28) return false;   // lab A/B: the fold-form exact policy
#endif
    const int t128 = ((M + 127) / 128) * (np / 256);
    if (horner_ready(hc, M)) return false;
    if (t128 >= kCUs) return true;
    if (np % 128 != 0 || hc->K % 256 != 0) return false;
    const int tk = ((M + 127) / 128) * (np / 128);   // the two-k-group 128 x 128 grid
    return 178 * ((t128 + kCUs - 1) / kCUs) <= 100 * ((tk + kCUs - 1) / kCUs);
}

// A 64-row grid of at least 3/4 of a round takes the two-k-group PC kernel: M 321..448 at N 4096
// (192..224 tiles) ran 21.3 / 21.4 us at M 384 / 448 against 21.8 / 23.4 for the 4-k-group fold
// tiles of mid M; at 5/8 of a round (M 300, 160 tiles) the fold tiles stay faster (21.4 vs 22.8 us;
// profiles/r06_tiles/pc_kg2_fill_ab.jsonl, 40-layer chain).
constexpr int kPcKg2MinFill = 3 * kCUs / 4;

// The two-k-group PC kernel (rows x 128 tiles, linear_pc.hip): where none of the larger Horner grids
// fills a round, 128- or 64-row tiles by rounds x tile time (below) (128: the 4-GPU
// column shard M = 4096 x N 1024, M = 2048 x N 2048, M = 1024 x N 4096: 34.8 -> 32.3 us; 64: M = 512
// x N 4096 and the 8-GPU shard 4096 x 512: 22.1 -> 21.5 us).  32-row tiles lose to the 4-k-group
// fold tiles at mid M (M 256: 17.1 vs 14.3 us; profiles/r06_tiles/).  Returns the tile rows, 0 = not
// applicable.
int horner_pc_kg2_rows(const PlanShape *hc, int M) {
    const int np = static_cast<int>(hc->Npad);
    if (!(hc->precision == DLLM_PRECISION_EXACT && hc->bits == 4 && hc->group == 128 && hc->K % 256 == 0 &&
          np % 128 == 0 && hc->horner_ok))
        return 0;
#if DLLM_LAB
    if (hc->variant == 14 || hc->variant == 28) return 0;   // lab A/B: the fold-form exact policy
#endif
    if (horner_ready(hc, M) || horner_pc_ready(hc, M) || horner_kg2_ready(hc, M)) return 0;
    // A 128-row tile takes ~1.55x a 64-row one (33 vs 21 us at K 4096: the 4- and 8-GPU shards), so
    // a grid of 128-row tiles short of a round still beats two rounds of 64-row tiles, and a single
    // round of 64-row tiles beats one of 128-row tiles.  N 4096: M 513..768 now take 128-row tiles
    // (M 700 / 768: 42.1 / 39.1 -> 33.3 / 30.5 us in the 40-layer chain; they took 64-row tiles in
    // 1.1 - 1.5 rounds) and M 321..448 64-row tiles (a 64-row grid of fewer than kPcKg2MinFill
    // tiles leaves mid M to the fold tiles); profiles/r06_tiles/pc_kg2_fill_ab.jsonl, pc_kg2_policy_ab.jsonl.
    const int t128 = ((M + 127) / 128) * (np / 128), t64 = ((M + 63) / 64) * (np / 128);
    if (t128 >= 2 * kCUs) return 0;   // the larger tiles of the other kernels fill the chip
    if (t128 >= kCUs || t64 > kCUs) return 128;
    return t64 >= kPcKg2MinFill ? 64 : 0;
}

}  // namespace

// The Horner kernel on 128-token tiles (wq_horner16_kernel<..., TB = 8>, x 256 columns, 128-deep
// stages), for grids where the 256 x 256 Horner grid leaves CUs idle but 128 x 256 tiles fill a round
// (M = 2048 at N = 4096; the 2-GPU column shard, M = 4096 x N 2048).  Lab A/B only (variant 323):
// against the fold form on those grids it measured -2.8 % on one box and +8 % on another (M = 2048:
// 64.9 vs 66.7 us, 72.5 vs 67.0 us; profiles/r04_horner/), so the fold form stays the product path.
// Returns the tile rows, 0 = not applicable.
#if DLLM_LAB
int horner_rows(const PlanShape *hc, int M) {
    const int np = static_cast<int>(hc->Npad);
    if (hc->variant != 323 || hc->bits != 4 || !horner_shape(hc) || !hc->horner_ok) return 0;
    if (((M + 127) / 128) * (np / 256) >= kCUs) return 128;
    return 0;
}
#endif

// ---- exact weights, fold form (linear_exact.hip) -----------------------------------------------

// The mid-M tiles also where their grid is short of a round (kMidMMinFill tiles and more): one
// 32 x 128 tile per CU takes the same time whether 96 or 256 CUs have one.  N 4096, 40-layer chain:
// M 65 / 96 / 128 / 160 / 192 / 224 = 16.5 / 18.2 / 20.4 / 23.1 / 24.6 / 23.5 -> 15.4 / 17.2 / 17.1 /
// 16.5 / 16.6 / 16.5 us against the K-split 64 x 128 tiles (profiles/r06_tiles/midm_short_grid_ab.jsonl);
// from 48 tiles (narrow N): N 2048 M 128 15.0 -> 13.2, N 1024 M 256 14.9 -> 13.2, N 512 M 384 / 512
// 13.7 / 15.0 -> 13.2 / 13.2 us, nothing slower (profiles/r06_tiles/m48/).
constexpr int kMidMMinFill = 48;

ExactGrids exact_grids(int M, int K, int Npad, int group) {
    ExactGrids g;
    const int mb = (M + 127) / 128;
    g.tiles = mb * (Npad / 128);
    g.t64 = ((M + 63) / 64) * (Npad / 128);
    g.t32 = ((M + 31) / 32) * (Npad / 128);
    g.ngroups = K / group;
    g.full256 = Npad % 256 == 0 && mb * (Npad / 256) >= kCUs;
    // Mid M: 32 x 128 tiles of 4 waves streaming the whole K -- no K split, hence no f32 slabs and
    // no combine launch -- where they give a full round but 64 x 128 tiles do not (M 225..448 at
    // N = 4096, where the policy below splits K): M 256 / 384: 25.1 -> 20.4 / 30.0 -> 24.6 us; at
    // M >= 512 the 64 x 128 two-k-group tiles stay faster (23.1 vs 25.8 us)
    // (profiles/r03_midm/policy_ab.json).
    g.mid = g.tiles < kCUs && g.t64 < kCUs && g.t32 >= kMidMMinFill;
    g.one_round = g.tiles >= kCUs && g.tiles < 2 * kCUs && g.ngroups % 2 == 0;
    return g;
}

int exact_split64(const ExactGrids &g, int K) {
    int ns = 1;
    while (g.t64 * ns < 2 * kCUs && ns < 8 && g.ngroups % (2 * ns) == 0 && (K / kBK) / (2 * ns) >= 4) ns *= 2;
    return ns;
}

// Fold-form tile policy (fills a DLLM_KERNEL_EXACT_FOLD plan; launch_exact_bits maps each plan to
// its template arguments).  Needs exact_gemm_supported(M, K, Npad, group).
// 1. 128 x 256 tiles (8 waves, two per SIMD; stages of one 128-row group) when they give >= 256
//    blocks; int4 g128: the two wave halves half a step apart (DLLM_PLAN_STAGGERED: M 2048 / 3072 x
//    4096: 76.9 -> 73.9 / 121.6 -> 114.0 us, same bits; profiles/r05_stag);
// 2. (int4 g128) the mid-M 32 x 128 tiles (exact_grids);
// 3. (int4 g128) 128 x 128 tiles with two k-groups per block when those give 256..511 blocks, else
//    64 x 128 tiles with two k-groups when those give >= 256 (4096 x 1024: 45.0 -> 40.5 us;
//    4096 x 512: 32.0 -> 24.4 us);
// 4. 64 x 128 tiles (4 waves) while 128 x 128 tiles give < 512 blocks, K split until >= 512;
// 5. 128 x 128 tiles (4 waves, two blocks per CU, 64-deep stages) with K split over group-aligned
//    slices until the grid has >= ~200 blocks.
void exact_plan(int bits, int M, int K, int Npad, int group, dllm_linear_plan_t *p) {
    // the int4 g128 forms: weight words in registers
    const bool i4g128 = group / kBK == 2 && bits == 4;
    const ExactGrids g = exact_grids(M, K, Npad, group);
    auto set = [&](int tm, int tn, int kg, int ns, int flags) {
        p->kernel = DLLM_KERNEL_EXACT_FOLD;
        p->tile_m = tm; p->tile_n = tn; p->kgroups = kg; p->nsplit = ns;
        p->flags = flags | (ns > 1 ? DLLM_PLAN_SPLITK : 0);
    };
    if (g.full256) return set(128, 256, 1, 1, i4g128 ? DLLM_PLAN_STAGGERED : 0);
    if (i4g128 && g.mid) {
        // k-groups of 4 waves sharing the tile (k-group g streams the g-th part of K; sums handed
        // to k-group 0 through the ring): four (16 waves, one block per CU) while the grid is
        // one block per CU, else two (8 waves, two blocks per CU fit).  M 256: 20.4 (one
        // k-group) -> 15.5 (two) -> 14.3 us (four); M 384: 24.5 -> 22.1 (two) / 25.1 (four)
        // (profiles/r03_midm/kgroups.jsonl).
        if (g.t32 <= kCUs && g.ngroups % 4 == 0) return set(32, 128, 4, 1, 0);
        if (g.ngroups % 2 == 0) return set(32, 128, 2, 1, 0);
        return set(32, 128, 1, 1, 0);
    }
    // tile-starved grids: 128 x 128 (or 64 x 128) tiles with two k-groups of 4 waves per block
    if (i4g128) {
        if (g.one_round) return set(128, 128, 2, 1, 0);
        if (g.tiles < kCUs && g.t64 >= kCUs && g.ngroups % 2 == 0) return set(64, 128, 2, 1, 0);
    }
    if (g.tiles < 2 * kCUs) return set(64, 128, 1, exact_split64(g, K), 0);
    int nsplit = 1;
    while (g.tiles * nsplit < 200 && nsplit < 8 && g.ngroups % (2 * nsplit) == 0 && (K / kBK) / (2 * nsplit) >= 4)
        nsplit *= 2;
    return set(128, 128, 1, nsplit, 0);
}

// ---- the selection -----------------------------------------------------------------------------

namespace {
// Prefill (M > kDecodeMaxM, or no decode layout): the exact-weight kernels (default precision) --
// the Horner family where its grids fit, else the fold-form tiles (exact_plan) -- or the rounded ring.
void prefill_plan(const PlanShape *h, int M, dllm_linear_plan_t *p) {
    if (!use_exact(h)) return rounded_plan(h, M, p);
    auto horner = [&](int kernel, int tm, int tn, int kg) {
        p->kernel = kernel;
        p->tile_m = tm; p->tile_n = tn; p->kgroups = kg; p->nsplit = 1;
        p->flags = 0;
    };
    if ((h->bits == 4 || h->bits == 2) && horner_ready(h, M)) return horner(DLLM_KERNEL_HORNER16, 256, 256, 1);
    if (h->bits == 4 && horner_pc_ready(h, M)) return horner(DLLM_KERNEL_HORNER_PC, 128, 256, 1);
    if (h->bits == 4 && horner_kg2_ready(h, M)) return horner(DLLM_KERNEL_HORNER_KG2, 256, 128, 2);
    if (const int rows = h->bits == 4 ? horner_pc_kg2_rows(h, M) : 0)
        return horner(DLLM_KERNEL_HORNER_PC_KG2, rows, 128, 2);
    exact_plan(h->bits, M, static_cast<int>(h->K), static_cast<int>(h->Npad), static_cast<int>(h->group), p);
}
}  // namespace

// The one kernel selection of the linear layer.  `fused`: the plan of
// dllm_linear_forward_psample(_ex), whose M <= kDecodeMaxM calls run the plain GEMM and the p_sample
// kernel.
void select_plan(const PlanShape *h, size_t M, int fused, dllm_linear_plan_t *p) {
    if (M <= static_cast<size_t>(kDecodeMaxM) && h->decode_layout) decode_plan(h, static_cast<int>(M), p);
    else prefill_plan(h, static_cast<int>(M), p);
    if (fused && M <= static_cast<size_t>(kDecodeMaxM)) p->flags |= DLLM_PLAN_NOT_FUSED;
}

}  // namespace dllm
