"""Every kernel the linear layer's dispatch can launch, at the smallest shape that reaches it.

Each case first asserts ``QuantLinear.plan`` (the dispatch's own selection, dllm_linear_plan), so a
case cannot silently run another kernel, then checks the result bit for bit:

* plain entry point: f32 output == the f64 product, f16 output == its RNE, and a second call into a
  NaN-filled output gives the same bits;
* fused p_sample entry point: x_prev == the oracle's p_sample on the exact eps with the oracle's own
  noise stream and coefficients (not the GPU's unfused pair), with rows_per_sample = 37, so output
  tiles straddle samples and the last sample is ragged -- in-lane noise, the ``noise=`` operand, in
  place, and with the f16 copy.

Data (``exact_layer``): random codes, random zero points in [0, 2^b - 1] and scales 2^e(g, n) with
e random in {-2..2} (int8: {-1..1}); X small integers (|x| <= 2, int8 <= 1), integer bias.  With
K max|x| (2^b - 1) 2^(2 (e_max - e_min)) < 2^24 every partial sum of every summation form is an
integer multiple of 2^e_min below 2^24 of them, hence exact in f32: the fold form (group sums times
scales), the Horner form (ratios are powers of two), the two-k-group hand-off and the split-K
combine.  A scale, zero point or ratio read from the wrong group or column changes the result.
``horner_ok = 0`` cases give one column a group of scale 2^-70 whose codes all equal its zero
point: create rejects the handle's ratios (the fold tiles run) and the column stays exact.

MATRIX is plain data and imports without a GPU: tests/test_linear_plan_cpu.py checks on any machine
that it covers every plan class the policy sweep reaches and that each entry's class is what
dllm_linear_plan_shape returns.  Shapes: per class the smallest (M, K, N) with M % 16 != 0, N % 8 ==
4 and a padded last column block (K as small as gives every k-group and K slice two groups, so
each chain rescales once), and for the prefill kernels an aligned one ("_a": whole tiles, N % 256 ==
0 or a multiple of the 128-column tile) for their LDS-coalesced f16 row stores.  HORNER_KG2 has no
whole-tile shape: it is only reached where ceil(M / 128) == ceil(M / 256), i.e. M <= 128 < its 256
rows."""
from collections import namedtuple

import numpy as np
import pytest

Case = namedtuple("Case", "id M K N bits group precision horner_ok prefill_only plan")

# plan = (kernel, tile_m, tile_n, kgroups, nsplit, flags) of the plain entry point
# (flags: 1 staggered, 2 decode X in LDS, 4 split-K combine follows).
MATRIX = [Case(*c) for c in [
    ("decode16", 5, 256, 124, 4, 128, 0, 1, 0, ("DECODE", 16, 16, 1, 1, 0)),
    ("decode16_g64", 7, 256, 124, 4, 64, 0, 1, 0, ("DECODE", 16, 16, 1, 1, 0)),
    ("decode16_f16w", 3, 256, 124, 4, 128, 1, 1, 0, ("DECODE", 16, 16, 1, 1, 0)),
    ("decode16_int2", 6, 256, 124, 2, 128, 0, 1, 0, ("DECODE", 16, 16, 1, 1, 0)),
    ("decode16_int8", 9, 256, 124, 8, 128, 0, 1, 0, ("DECODE", 16, 16, 1, 1, 0)),
    ("decode16_xl", 13, 1024, 124, 4, 128, 0, 1, 0, ("DECODE", 16, 16, 1, 1, 2)),
    ("decode16_xl_int8", 11, 1024, 124, 8, 256, 0, 1, 0, ("DECODE", 16, 16, 1, 1, 2)),
    ("decode32", 23, 256, 124, 4, 128, 0, 1, 0, ("DECODE", 32, 16, 1, 1, 0)),
    ("decode64_split", 50, 1024, 252, 4, 128, 0, 1, 0, ("DECODE", 64, 64, 1, 4, 4)),
    ("decode64_split_int2", 37, 1024, 252, 2, 128, 0, 1, 0, ("DECODE", 64, 64, 1, 4, 4)),
    ("prefill_only_fold64", 37, 256, 124, 4, 128, 0, 1, 1, ("EXACT_FOLD", 64, 128, 1, 1, 0)),
    ("prefill_only_fold64_split", 37, 512, 124, 4, 128, 0, 1, 1, ("EXACT_FOLD", 64, 128, 1, 2, 4)),
    ("prefill_only_mid_kg2", 37, 768, 8188, 4, 128, 0, 1, 1, ("EXACT_FOLD", 32, 128, 2, 1, 0)),
    ("prefill_only_mid_kg4", 50, 1024, 8188, 4, 128, 0, 1, 1, ("EXACT_FOLD", 32, 128, 4, 1, 0)),
    ("fold64_int8", 70, 256, 124, 8, 128, 0, 1, 0, ("EXACT_FOLD", 64, 128, 1, 1, 0)),
    ("fold64_int2_a", 128, 256, 256, 2, 128, 0, 1, 0, ("EXACT_FOLD", 64, 128, 1, 1, 0)),
    ("fold64_split4", 70, 1024, 124, 4, 128, 0, 1, 0, ("EXACT_FOLD", 64, 128, 1, 4, 4)),
    ("fold64_split_int8_a", 128, 1024, 256, 8, 64, 0, 1, 0, ("EXACT_FOLD", 64, 128, 1, 4, 4)),
    ("mid_kg1", 70, 384, 8188, 4, 128, 0, 1, 0, ("EXACT_FOLD", 32, 128, 1, 1, 0)),
    ("mid_kg1_a", 768, 384, 256, 4, 128, 0, 1, 0, ("EXACT_FOLD", 32, 128, 1, 1, 0)),
    ("mid_kg2_nohorner", 193, 768, 4092, 4, 128, 0, 0, 0, ("EXACT_FOLD", 32, 128, 2, 1, 0)),
    ("mid_kg2_a", 768, 768, 256, 4, 128, 0, 1, 0, ("EXACT_FOLD", 32, 128, 2, 1, 0)),
    ("mid_kg4_nohorner", 100, 1024, 8188, 4, 128, 0, 0, 0, ("EXACT_FOLD", 32, 128, 4, 1, 0)),
    ("mid_kg4_a", 768, 1024, 256, 4, 128, 0, 1, 0, ("EXACT_FOLD", 32, 128, 4, 1, 0)),
    ("fold64_kg2_nohorner", 193, 512, 8188, 4, 128, 0, 0, 0, ("EXACT_FOLD", 64, 128, 2, 1, 0)),
    ("fold64_kg2_nohorner_a", 8192, 512, 256, 4, 128, 0, 0, 0, ("EXACT_FOLD", 64, 128, 2, 1, 0)),
    ("fold128_kg2_nohorner", 401, 512, 8188, 4, 128, 0, 0, 0, ("EXACT_FOLD", 128, 128, 2, 1, 0)),
    ("fold128_kg2_nohorner_a", 8192, 512, 512, 4, 128, 0, 0, 0, ("EXACT_FOLD", 128, 128, 2, 1, 0)),
    ("fold128", 2057, 256, 3964, 4, 128, 0, 1, 0, ("EXACT_FOLD", 128, 128, 1, 1, 0)),
    ("fold128_a", 2176, 256, 3968, 4, 128, 0, 1, 0, ("EXACT_FOLD", 128, 128, 1, 1, 0)),
    ("fold128x256_stag_nohorner", 129, 256, 32764, 4, 128, 0, 0, 0, ("EXACT_FOLD", 128, 256, 1, 1, 1)),
    ("fold128x256_stag_nohorner_a", 8192, 256, 1024, 4, 128, 0, 0, 0, ("EXACT_FOLD", 128, 256, 1, 1, 1)),
    ("fold128x256_g64", 129, 256, 32764, 4, 64, 0, 1, 0, ("EXACT_FOLD", 128, 256, 1, 1, 0)),
    ("fold128x256_int2", 131, 256, 32764, 2, 128, 0, 1, 0, ("EXACT_FOLD", 128, 256, 1, 1, 0)),
    ("fold128x256_int8_a", 8192, 256, 1024, 8, 128, 0, 1, 0, ("EXACT_FOLD", 128, 256, 1, 1, 0)),
    ("horner16", 2689, 256, 3068, 4, 128, 0, 1, 0, ("HORNER16", 256, 256, 1, 1, 0)),
    ("horner16_a", 2816, 256, 3072, 4, 128, 0, 1, 0, ("HORNER16", 256, 256, 1, 1, 0)),
    ("horner16_int2", 2689, 256, 3068, 2, 128, 0, 1, 0, ("HORNER16", 256, 256, 1, 1, 0)),
    ("horner16_int2_a", 2816, 256, 3072, 2, 128, 0, 1, 0, ("HORNER16", 256, 256, 1, 1, 0)),
    ("horner_pc", 1281, 256, 3068, 4, 128, 0, 1, 0, ("HORNER_PC", 128, 256, 1, 1, 0)),
    ("horner_pc_a", 4224, 256, 1024, 4, 128, 0, 1, 0, ("HORNER_PC", 128, 256, 1, 1, 0)),
    ("horner_pc_m4300", 4300, 256, 4096, 4, 128, 0, 1, 0, ("HORNER_PC", 128, 256, 1, 1, 0)),
    ("horner_kg2", 100, 512, 32764, 4, 128, 0, 1, 0, ("HORNER_KG2", 256, 128, 2, 1, 0)),
    ("horner_kg2_corner", 100, 512, 32768, 4, 128, 0, 1, 0, ("HORNER_KG2", 256, 128, 2, 1, 0)),
    ("horner_pc_kg2_128", 641, 512, 3068, 4, 128, 0, 1, 0, ("HORNER_PC_KG2", 128, 128, 2, 1, 0)),
    ("horner_pc_kg2_128_a", 4224, 512, 512, 4, 128, 0, 1, 0, ("HORNER_PC_KG2", 128, 128, 2, 1, 0)),
    ("horner_pc_kg2_64", 129, 512, 8188, 4, 128, 0, 1, 0, ("HORNER_PC_KG2", 64, 128, 2, 1, 0)),
    ("horner_pc_kg2_64_a", 6144, 512, 256, 4, 128, 0, 1, 0, ("HORNER_PC_KG2", 64, 128, 2, 1, 0)),
    ("ring128", 70, 256, 124, 4, 128, 1, 1, 0, ("ROUNDED_RING", 128, 128, 2, 1, 0)),
    ("ring128_a", 128, 256, 256, 8, 128, 1, 1, 0, ("ROUNDED_RING", 128, 128, 2, 1, 0)),
    ("ring128_split", 70, 512, 124, 4, 128, 1, 1, 0, ("ROUNDED_RING", 128, 128, 2, 2, 4)),
    ("ring128_split_a", 128, 512, 256, 2, 128, 1, 1, 0, ("ROUNDED_RING", 128, 128, 2, 2, 4)),
    ("ring128_exact_partial_group", 70, 384, 124, 4, 256, 0, 1, 0, ("ROUNDED_RING", 128, 128, 2, 1, 0)),
    ("ring256x128", 70, 256, 32764, 4, 128, 1, 1, 0, ("ROUNDED_RING", 256, 128, 2, 1, 0)),
    ("ring256x128_a", 8192, 256, 1024, 4, 128, 1, 1, 0, ("ROUNDED_RING", 256, 128, 2, 1, 0)),
    ("ring256", 257, 256, 32764, 4, 128, 1, 1, 0, ("ROUNDED_RING", 256, 256, 1, 1, 0)),
    ("ring256_a", 8192, 256, 2048, 4, 128, 1, 1, 0, ("ROUNDED_RING", 256, 256, 1, 1, 0)),
]]

PLAN_NOT_FUSED = 8
ROWS_PER_SAMPLE = 37


def plan_class(plan):
    """(kernel, tile_m, tile_n, kgroups, nsplit > 1, flags) of a plan tuple: what the coverage guard counts."""
    kernel, tile_m, tile_n, kgroups, nsplit, flags = plan
    return (kernel, tile_m, tile_n, kgroups, nsplit > 1, flags & ~PLAN_NOT_FUSED)


def exact_layer(case, seed):
    """-> codes [K, N] u8, scales [G, N] f32, zps [G, N] u8, bias [N] f32, X [M, K] f32, and the f64
    product Y = X . ((codes - zp) * scale) + bias, with the exactness condition asserted."""
    M, K, N, bits, group = case.M, case.K, case.N, case.bits, case.group
    rng = np.random.default_rng(seed)
    q, G = (1 << bits) - 1, (K + group - 1) // group
    emax, xmax = (1, 1) if bits == 8 else (2, 2)
    assert K * xmax * q * 2 ** (2 * (2 * emax)) < 2 ** 24, "partial sums must stay exact in f32"
    codes = rng.integers(0, q + 1, (K, N), dtype=np.uint8)
    zps = rng.integers(0, q + 1, (G, N), dtype=np.uint8)
    scales = np.exp2(rng.integers(-emax, emax + 1, (G, N))).astype(np.float32)
    if not case.horner_ok:   # a group of scale 2^-70 that contributes exactly 0: the ratios are rejected
        g, n = G - 1, 5
        scales[g, n] = np.float32(2.0 ** -70)
        codes[g * group:(g + 1) * group, n] = zps[g, n]
    X = rng.integers(-xmax, xmax + 1, (M, K)).astype(np.float32)
    bias = rng.integers(-4, 5, N).astype(np.float32)
    rows = np.arange(K) // group
    W = (codes.astype(np.float64) - zps[rows].astype(np.float64)) * scales[rows].astype(np.float64)
    Y = X.astype(np.float64) @ W + bias
    assert np.array_equal(Y.astype(np.float32).astype(np.float64), Y) and np.abs(Y).max() < 65504
    return codes, scales, zps, bias, X, Y


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch(cuda):
    import torch as t
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


@pytest.fixture(scope="module")
def built():
    """The latest case's (handle, device X, f64 reference): its plain and fused runs share them."""
    cache = {}
    yield cache
    for old in cache.values():
        old[0].close()


def build(dllm, torch, orc, case, _built):
    """The case's handle, device X and f64 reference, built once (only the latest case is kept)."""
    if case.id not in _built:
        for old in _built.values():
            old[0].close()
        _built.clear()
        codes, scales, zps, bias, X, Y = exact_layer(case, seed=len(case.id) + case.M + case.N + case.bits)
        lin = dllm.QuantLinear.from_quantized(dev(torch, orc.pack_bits(codes.ravel(), case.bits)), dev(torch, scales),
                                              dev(torch, zps), case.K, case.N, case.bits, case.group,
                                              bias=dev(torch, bias), precision=case.precision,
                                              prefill_only=bool(case.prefill_only))
        _built[case.id] = (lin, dev(torch, X).half(), Y)
    return _built[case.id]


def check_plan(lin, case, fused):
    got = lin.plan(case.M, fused=fused).astuple()
    want = case.plan[:5] + (case.plan[5] | (PLAN_NOT_FUSED if fused and case.M <= 64 else 0),)
    assert got == want, (case.id, fused, got, want)


def run_plain(dllm, torch, orc, case, built):
    lin, Xd, Y = build(dllm, torch, orc, case, built)
    check_plan(lin, case, fused=False)
    ref32 = Y.astype(np.float32)
    ref16 = ref32.astype(np.float16)
    y32 = host(lin(Xd, out_dtype=torch.float32))
    bad = np.argwhere(bits_of(y32) != bits_of(ref32))
    assert bad.size == 0, (case.id, "f32", len(bad), bad[:4].tolist())
    y16 = host(lin(Xd, out_dtype=torch.float16))
    bad = np.argwhere(bits_of(y16) != bits_of(ref16))
    assert bad.size == 0, (case.id, "f16", len(bad), bad[:4].tolist())
    for ref, dt in ((ref32, torch.float32), (ref16, torch.float16)):   # every element is written, again the same
        out = torch.full((case.M, case.N), float("nan"), device="cuda", dtype=dt)
        lin(Xd, out=out)
        assert np.array_equal(bits_of(host(out)), bits_of(ref)), (case.id, "second call", str(dt))


def run_fused(dllm, torch, orc, case, built, rps):
    lin, Xd, Y = build(dllm, torch, orc, case, built)
    check_plan(lin, case, fused=True)
    M, N = case.M, case.N
    S = (M + rps - 1) // rps
    seed, offset = 11, 4 * (case.M + 3)
    betas = dllm.DiffusionConfig().create_beta_schedule()
    coef = orc.p_sample_coeffs(betas, [999 - 7 * i % 990 for i in range(S)], inclusive=True)   # every t > 0: noise is added
    x_t = np.random.default_rng(M + N).standard_normal((M, N)).astype(np.float32)
    noise = orc.randn(seed, offset, M * N).reshape(M, N)
    ref = orc.p_sample(x_t, Y.astype(np.float32), noise, np.repeat(coef, rps, axis=0)[:M], add_noise=True)
    ref16 = ref.astype(np.float16)
    xt_d, coef_d = dev(torch, x_t), dev(torch, coef)

    def same(t, what):
        bad = np.argwhere(bits_of(host(t)) != bits_of(ref))
        assert bad.size == 0, (case.id, rps, what, len(bad), bad[:4].tolist())

    same(lin.forward_psample(Xd, xt_d, coef_d, rps, True, seed, offset), "in-lane noise")
    same(lin.forward_psample(Xd, xt_d, coef_d, rps, True, 0, 0, noise=dev(torch, noise)), "noise operand")
    xt2 = xt_d.clone()
    lin.forward_psample(Xd, xt2, coef_d, rps, True, seed, offset, out=xt2)
    same(xt2, "in place")
    h16 = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float16)
    out = torch.full((M, N), float("nan"), device="cuda")
    lin.forward_psample(Xd, xt_d, coef_d, rps, True, seed, offset, out=out, out16=h16)
    same(out, "with out16")
    assert np.array_equal(bits_of(host(h16)), bits_of(ref16)), (case.id, rps, "out16")


# (case, entry): a case's plain and fused runs are adjacent, so its handle and reference are built once.
RUNS = [(c, e) for c in MATRIX for e in (("plain", "fused", "fused_rps1") if c.M <= 64 else ("plain", "fused"))]


@pytest.mark.parametrize("case,entry", RUNS, ids=[f"{c.id}-{e}" for c, e in RUNS])
def test_linear_kernel(dllm, torch, orc, built, case, entry):
    """One MATRIX case through dllm_linear_forward (``plain``) or dllm_linear_forward_psample_ex
    (``fused``: rows_per_sample 37; ``fused_rps1``, M <= 64 only: one row per sample, no coefficient
    expansion), bit-equal to the f64 product / the oracle's p_sample of it (module docstring)."""
    if entry == "plain":
        run_plain(dllm, torch, orc, case, built)
    else:
        assert case.N % 4 == 0
        run_fused(dllm, torch, orc, case, built, 1 if entry == "fused_rps1" else ROWS_PER_SAMPLE)
