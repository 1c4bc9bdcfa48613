"""GPU parity of the diffusion-step kernels against the C oracle: the seeded
noise stream, p_sample and add_noise bit for bit, the GEMM-fused p_sample epilogue bit-identical
to the unfused pair on every GEMM path, the phase-aware KV cache, and the denoise loop against
an f32 torch restatement."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("seed,offset,n", [(0, 0, 1 << 20), (1234, 4, 4099), (2**63 + 7, 1 << 40, 77), (5, 8, 3)])
def test_randn_bit_exact(dllm, cuda, orc, seed, offset, n):
    import torch
    z = dllm.randn(n, seed, offset).cpu().numpy()
    assert np.array_equal(bits(z), bits(orc.randn(seed, offset, n)))


@pytest.mark.parametrize("B,D", [(6, 64), (3, 1001), (1, 4096 * 33)])
@pytest.mark.parametrize("cumprod", [0, 1])
def test_p_sample_bit_exact(dllm, cuda, orc, B, D, cumprod):
    import torch
    cfg = dllm.DiffusionConfig(num_timesteps=1000)
    rng = np.random.default_rng(B * D)
    x = rng.standard_normal((B, D)).astype(np.float32)
    eps = rng.standard_normal((B, D)).astype(np.float32)
    t = [999, 0, 1, 500, 2, 3][:B]
    coef = orc.p_sample_coeffs(cfg.create_beta_schedule(), t, cumprod)
    flag = t[0] > 0
    # generated noise (seeded stream, offset 8)
    y = dllm.p_sample(cfg, torch.from_numpy(x), t, torch.from_numpy(eps), seed=77, offset=8,
                      cumprod=dllm.Cumprod(cumprod)).cpu().numpy()
    ref = orc.p_sample(x, eps, orc.randn(77, 8, B * D).reshape(B, D), coef, add_noise=flag)
    assert same(y, ref)
    # caller-supplied noise
    nz = rng.standard_normal((B, D)).astype(np.float32)
    y2 = dllm.p_sample(cfg, torch.from_numpy(x), t, torch.from_numpy(eps), noise=torch.from_numpy(nz),
                       cumprod=dllm.Cumprod(cumprod)).cpu().numpy()
    assert same(y2, orc.p_sample(x, eps, nz, coef, add_noise=flag))


def test_p_sample_last_step_without_noise(dllm, cuda, orc):
    """t[0] == 0: the reference adds zeros (lib.rs:1198-1204); inclusive form, finite result."""
    import torch
    cfg = dllm.DiffusionConfig()
    x = np.random.default_rng(1).standard_normal((2, 128)).astype(np.float32)
    e = np.random.default_rng(2).standard_normal((2, 128)).astype(np.float32)
    y = dllm.p_sample(cfg, torch.from_numpy(x), [0, 0], torch.from_numpy(e), seed=3,
                      cumprod=dllm.Cumprod.INCLUSIVE).cpu().numpy()
    coef = orc.p_sample_coeffs(cfg.create_beta_schedule(), [0, 0], inclusive=True)
    assert same(y, orc.p_sample(x, e, None, coef, add_noise=False)) and np.isfinite(y).all()


@pytest.mark.parametrize("cumprod", [0, 1])
def test_add_noise_bit_exact(dllm, cuda, orc, cumprod):
    import torch
    cfg = dllm.DiffusionConfig()
    rng = np.random.default_rng(11)
    x0 = rng.standard_normal((4, 515)).astype(np.float32)
    t = [0, 10, 999, 2000]
    noisy, nz = dllm.add_noise(cfg, torch.from_numpy(x0), t, seed=9, offset=4, cumprod=dllm.Cumprod(cumprod))
    ref_nz = orc.randn(9, 4, x0.size).reshape(x0.shape)
    assert np.array_equal(bits(nz.cpu().numpy()), bits(ref_nz))
    coef = orc.add_noise_coeffs(cfg.create_beta_schedule(), t, cumprod)
    assert same(noisy.cpu().numpy(), orc.add_noise(x0, ref_nz, coef))
    n2, _ = dllm.add_noise(cfg, torch.from_numpy(x0), t, noise=torch.from_numpy(ref_nz), cumprod=dllm.Cumprod(cumprod))
    assert same(n2.cpu().numpy(), orc.add_noise(x0, ref_nz, coef))


# (M, K, N, rows_per_sample), exact / rounded weights: decode path (unfused, both), the fold form's
# 32 x 128 four-k-group tiles / the 128 x 128 ring with split-K (fused in the combine), the
# two-k-group producer/consumer 128 x 128 tiles / the 128 x 128 ring (M 1024 and 4096 x N 1024), the
# producer/consumer 128 x 256 tiles / the 256 x 128 ring, the 256 x 256 Horner tiles / 256 x 256 ring
# -- all with the fused entry point vs forward(f32) + p_sample.  (Every fused epilogue at ragged
# shapes and the other widths, against the oracle: tests/test_gpu_linear_kernels.py.)
PSAMPLE_KERNELS = {48: ("DECODE", "DECODE"), 256: ("EXACT_FOLD", "ROUNDED_RING"), 1024: ("HORNER_PC_KG2", "ROUNDED_RING"),
                   2048: ("HORNER_PC", "ROUNDED_RING"), 4096: ("HORNER16", "ROUNDED_RING")}


@pytest.mark.parametrize("M,K,N,rps", [(48, 512, 256, 16), (256, 1024, 4096, 64), (1024, 256, 4096, 1024),
                                       (2048, 256, 4096, 512), (4096, 256, 4096, 4096), (4096, 512, 1024, 2048)])
@pytest.mark.parametrize("precision", [0, 1])
def test_linear_psample_fused_bit_identical(dllm, cuda, M, K, N, rps, precision):
    import torch
    g = torch.Generator(device="cuda").manual_seed(M + K)
    W = 0.05 * torch.randn(K, N, device="cuda", generator=g)
    b = 0.1 * torch.randn(N, device="cuda", generator=g)
    lin = dllm.QuantLinear.from_weight(W, b, 4, 128, precision)
    want = PSAMPLE_KERNELS[M][precision] if N == 4096 or M == 48 else ("HORNER_PC_KG2", "ROUNDED_RING")[precision]
    plan = lin.plan(M, fused=True)
    assert plan.astuple()[0] == want and bool(plan.flags & dllm._lib.PLAN_NOT_FUSED) == (M <= 64), plan
    X = torch.randn(M, K, device="cuda", generator=g).half()
    xt = torch.randn(M, N, device="cuda", generator=g)
    S = M // rps
    cfg = dllm.DiffusionConfig()
    t = [999 - 7 * i for i in range(S)]
    coef_np, flag = dllm.diffusion.p_sample_coeffs(cfg, t, S, dllm.Cumprod.INCLUSIVE)
    coef = torch.from_numpy(coef_np).cuda()
    fused = lin.forward_psample(X, xt, coef, rps, flag, seed=5, offset=16)
    eps = lin(X, out_dtype=torch.float32)
    ref = torch.empty_like(xt)
    row_coef = coef.repeat_interleave(rps, dim=0).contiguous()
    lib = dllm._lib.load()
    dllm._lib.check(lib.dllm_p_sample(C.c_void_p(xt.data_ptr()), C.c_void_p(eps.data_ptr()), None,
                                      C.c_void_p(row_coef.data_ptr()), M, N, int(flag), 5, 16,
                                      C.c_void_p(ref.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(fused.view(torch.int32), ref.view(torch.int32))
    # in place (x_prev aliases x_t)
    xt2 = xt.clone()
    lin.forward_psample(X, xt2, coef, rps, flag, seed=5, offset=16, out=xt2)
    assert torch.equal(xt2.view(torch.int32), ref.view(torch.int32))
    # with the f16 copy of x_prev (dllm_linear_forward_psample_ex): the same f32 bits, and the f16
    # copy is the RNE of them, as a first layer's own cast of an f32 X
    h16 = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float16)
    xt3 = xt.clone()
    lin.forward_psample(X, xt3, coef, rps, flag, seed=5, offset=16, out=xt3, out16=h16)
    assert torch.equal(xt3.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(h16.view(torch.int16), ref.half().view(torch.int16))
    lin.close()


def test_kv_cache_entry_phases(dllm, cuda, orc):
    import torch
    rng = np.random.default_rng(3)
    K = rng.standard_normal((1, 64, 256)).astype(np.float32)
    V = rng.standard_normal((1, 64, 256)).astype(np.float32)
    c = dllm.KVCacheEntry.new(torch.from_numpy(K).cuda(), torch.from_numpy(V).cuda(), 8, 4)
    assert c.is_prefill_phase and c.get_current_quant_bits() == 8 and len(c) == 64
    q, s, z = orc.quantize_tensor(K, 8)
    assert np.array_equal(bits(c.get_keys().cpu().numpy().ravel()), bits(orc.dequantize_tensor(q, s, z)))
    c.set_phase(False)
    assert c.get_current_quant_bits() == 4
    q, s, z = orc.quantize_tensor(V, 4)
    assert np.array_equal(bits(c.get_values().cpu().numpy().ravel()), bits(orc.dequantize_tensor(q, s, z)))
    # lib.rs:279-302 accounting: packed K+V at 8 and at 4 bits
    n = K.size
    assert c.memory_usage() == 2 * n + 2 * ((n * 4 + 7) // 8)
    K2 = K + 1.0
    c.update(torch.from_numpy(K2).cuda(), torch.from_numpy(V).cuda())
    q, s, z = orc.quantize_tensor(K2, 4)
    assert np.array_equal(bits(c.get_keys().cpu().numpy().ravel()), bits(orc.dequantize_tensor(q, s, z)))


def test_denoise_loop_vs_torch_f32(dllm, cuda, orc):
    """A 3-layer loop (d = 512, M = 256 tokens, 6 steps, inclusive alpha-bar) against the same
    recursion in torch f32 on the exported dequantized weights, f16 activations between layers
    and the oracle's noise stream: tolerance 2e-3 relative on the final state."""
    import torch
    d, M, L, steps = 512, 256, 3, 6
    g = torch.Generator(device="cuda").manual_seed(0)
    Ws = [0.04 * torch.randn(d, d, device="cuda", generator=g) for _ in range(L)]
    layers = [dllm.QuantLinear.from_weight(W, None, 4, 128) for W in Ws]
    cfg = dllm.DiffusionConfig(num_timesteps=steps, beta_start=0.01, beta_end=0.2)
    loop = dllm.DenoiseLoop(layers, cfg, cumprod=dllm.Cumprod.INCLUSIVE, seed=21)
    x0 = torch.randn(M, d, device="cuda", generator=g)
    out = loop.sample(x0.clone(), steps)
    Wh = []
    for lin in layers:
        codes, s, z = lin.export()
        cd = orc.unpack_bits(codes.cpu().numpy(), d * d, 4).reshape(d, d)
        Wh.append(torch.from_numpy(orc.dequantize_weights(cd, s.cpu().numpy(), z.cpu().numpy(), 128)).cuda())
    x = x0.clone()
    for i, t in enumerate(range(steps - 1, -1, -1)):
        h = x
        for j, W in enumerate(Wh):
            h = h.half().float() @ W
            if j < L - 1:
                h = h.half().float()
        coef, flag = dllm.diffusion.p_sample_coeffs(cfg, [t], 1, dllm.Cumprod.INCLUSIVE)
        c1, c2, sd = (float(v) for v in coef[0])
        nz = torch.from_numpy(orc.randn(21, i * M * d, M * d).reshape(M, d)).cuda() if flag else 0.0
        x = (c1 * x + c2 * h) + sd * nz
    rel = (torch.linalg.norm(out - x) / torch.linalg.norm(x)).item()
    assert rel <= 2e-3, rel


@pytest.mark.parametrize("M", [48, 192])
def test_denoise_loop_overlap_bit_identical(dllm, cuda, M):
    """The overlapped schedule (KV update on the side stream; the last layer's epilogue also writes
    x_prev in f16 for the next step's first layer -- from the fused epilogue at M 192, from the
    p_sample + cast path at M 48) gives the same bits as the serial loop, and the KV cache ends in
    the same state."""
    import torch
    d, L, steps = 256, 2, 5
    g = torch.Generator(device="cuda").manual_seed(4)
    layers = [dllm.QuantLinear.from_weight(0.04 * torch.randn(d, d, device="cuda", generator=g), None, 4, 128)
              for _ in range(L)]
    cfg = dllm.DiffusionConfig(num_timesteps=steps, beta_start=0.01, beta_end=0.2)
    x0 = torch.randn(M, d, device="cuda", generator=g)
    K = torch.randn(1, 64, d, device="cuda", generator=g)
    outs, kvs = [], []
    for overlap in (False, True):
        kv = dllm.KVCacheEntry.new(K.clone(), K.clone() * 2, 8, 4)
        loop = dllm.DenoiseLoop(layers, cfg, cumprod=dllm.Cumprod.INCLUSIVE, seed=3, kv_cache=kv, overlap=overlap)
        outs.append(loop.sample(x0.clone(), steps))
        kvs.append(kv.get_keys())
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(kvs[0], kvs[1])


def test_denoise_loop_config5_full_size(dllm, cuda, orc):
    """Config C5 at its full size on one GPU: 12 int4 layers d = 4096, seq 2048, 50 steps with the
    phase-aware KV cache (8 / 4 bits, progressive precision on, the reference default) updated
    every step on the side stream and p_sample fused into the last layer.  Reference: the same
    recursion in torch f32 on the oracle-dequantized weights with f16 activations between layers,
    and the noise stream (checked bit-exact against the oracle in test_randn_bit_exact).  Weights
    0.5/sqrt(d) N(0,1) keep the state finite over the 50 steps; tolerance 2e-3 relative on the
    final state (50 compounded steps; the per-step bar is test_denoise_loop_config5_per_step).
    The KV cache ends in the state the oracle's KVCacheEntry restatement reaches: progressive
    precision has driven the decode width to 0, so get_keys hands out the f32 keys."""
    import torch
    d, M, L, steps, seed = 4096, 2048, 12, 50, 5
    g = torch.Generator(device="cuda").manual_seed(5)
    layers = [dllm.QuantLinear.from_weight((0.5 / 64.0) * torch.randn(d, d, device="cuda", generator=g), None, 4, 128)
              for _ in range(L)]
    cfg = dllm.DiffusionConfig(num_timesteps=steps, hidden_size=d, num_layers=L)
    assert cfg.progressive_precision
    K = torch.randn(1, M, d, device="cuda", generator=g)
    V = torch.randn(1, M, d, device="cuda", generator=g)
    kv = dllm.KVCacheEntry.new(K, V, cfg.prefill_bits, cfg.decode_bits)
    loop = dllm.DenoiseLoop(layers, cfg, cumprod=dllm.Cumprod.INCLUSIVE, seed=seed, kv_cache=kv)
    x0 = torch.randn(M, d, device="cuda", generator=g)
    out = loop.sample(x0.clone(), steps)
    assert bool(torch.isfinite(out).all())
    Wh = []
    for lin in layers:
        codes, s, z = lin.export()
        cd = orc.unpack_bits(codes.cpu().numpy(), d * d, 4).reshape(d, d)
        Wh.append(torch.from_numpy(orc.dequantize_weights(cd, s.cpu().numpy(), z.cpu().numpy(), 128)).cuda())
    x = x0.clone()
    for i, t in enumerate(range(steps - 1, -1, -1)):
        h = x
        for j, W in enumerate(Wh):
            h = h.half().float() @ W
            if j < L - 1:
                h = h.half().float()
        coef, flag = dllm.diffusion.p_sample_coeffs(cfg, [t], 1, dllm.Cumprod.INCLUSIVE)
        c1, c2, sd = (float(v) for v in coef[0])
        nz = dllm.randn(M * d, seed, i * M * d).reshape(M, d) if flag else 0.0
        x = (c1 * x + c2 * h) + sd * nz
    rel = (torch.linalg.norm(out - x) / torch.linalg.norm(x)).item()
    assert rel <= 2e-3, rel
    assert kv.decode_quant_bits == 0 and kv.decode_quantized is None and not kv.is_prefill_phase
    assert torch.equal(kv.get_keys(), K) and torch.equal(kv.get_values(), V)
    # the prefill copy is the last re-quantization of the pass-through K at 8 bits
    q, sc, zp = orc.quantize_tensor(K.cpu().numpy().ravel(), 8)
    kv.is_prefill_phase = True
    assert np.array_equal(kv.get_keys().cpu().numpy().ravel().view(np.uint32),
                          orc.dequantize_tensor(q, sc, zp).view(np.uint32))


def test_kv_cache_progressive_sequence_bitexact(dllm, cuda, orc):
    """The KV half of DiffuseLLM::sample with progressive precision on (lib.rs:884-918), 50 steps:
    at every step the width in use and the K/V handed to forward_with_cache are bit-identical
    to the oracle's KVCacheEntry restatement (phase switch at t = 25, decode widths 4 -> 2 -> 1
    -> 0, where the reference hands out the f32 K/V instead of asserting)."""
    import torch
    steps = 50
    g = torch.Generator(device="cuda").manual_seed(8)
    K = torch.randn(1, 256, 1024, device="cuda", generator=g) * 3 + 0.5
    V = torch.randn(1, 256, 1024, device="cuda", generator=g)
    cfg = dllm.DiffusionConfig(num_timesteps=steps)
    kv = dllm.KVCacheEntry.new(K, V, cfg.prefill_bits, cfg.decode_bits)
    loop = dllm.DenoiseLoop([], cfg, kv_cache=kv)
    ref = orc.KVCacheEntryRef(K.cpu().numpy(), V.cpu().numpy(), cfg.prefill_bits, cfg.decode_bits)
    widths = []
    for t in range(steps - 1, -1, -1):
        k, v = loop.kv_step(t, steps)
        rk, rv = orc.sample_kv_step(ref, t, steps, cfg.decode_bits, cfg.min_decode_bits)
        assert kv.is_prefill_phase == ref.is_prefill_phase and kv.decode_quant_bits == ref.decode_quant_bits
        assert np.array_equal(k.cpu().numpy().view(np.uint32), rk.view(np.uint32)), t
        assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32)), t
        widths.append(kv.get_current_quant_bits())
    assert widths == [8] * 24 + [2] + [1] * 12 + [0] * 13


def test_denoise_loop_config5_per_step(dllm, cuda, orc):
    """BASELINE.md's C5 bar, per step, teacher-forced: at each of the 50 steps of the full C5 loop
    (12 int4 layers d 4096, seq 2048, progressive KV precision on) the GPU step maps x_t to
    x_{t-1}; the reference maps the SAME x_t through the f32 chain on the oracle-dequantized
    weights (x.dot(W) per layer, lib.rs:806-813, then p_sample with the same noise).  Weights
    1/sqrt(d) N(0,1) keep every layer's gain near 1, so eps is as large as x and x_{t-1} ~ 0.96
    eps: the step's error is the 12-layer chain's.  Asserted: every step <= 1e-3 against the f32
    chain; the per-step errors are also written to gpurun_out/c5_per_step.json."""
    import json
    import os
    import torch
    d, M, L, steps, seed = 4096, 2048, 12, 50, 7
    g = torch.Generator(device="cuda").manual_seed(7)
    layers = [dllm.QuantLinear.from_weight((1.0 / 64.0) * torch.randn(d, d, device="cuda", generator=g), None, 4, 128)
              for _ in range(L)]
    cfg = dllm.DiffusionConfig(num_timesteps=steps, hidden_size=d, num_layers=L)
    K = torch.randn(1, M, d, device="cuda", generator=g)
    kv = dllm.KVCacheEntry.new(K, K * 0.5, cfg.prefill_bits, cfg.decode_bits)
    loop = dllm.DenoiseLoop(layers, cfg, cumprod=dllm.Cumprod.INCLUSIVE, seed=seed, kv_cache=kv, overlap=False)
    Wh = []
    for lin in layers:
        codes, s, z = lin.export()
        cd = orc.unpack_bits(codes.cpu().numpy(), d * d, 4).reshape(d, d)
        Wh.append(torch.from_numpy(orc.dequantize_weights(cd, s.cpu().numpy(), z.cpu().numpy(), 128)).cuda())
    x = torch.randn(M, d, device="cuda", generator=g)
    errs, errs16 = [], []
    for i, t in enumerate(range(steps - 1, -1, -1)):
        loop.kv_step(t, steps)
        x_next = loop.step(x, t, i)
        coef, flag = dllm.diffusion.p_sample_coeffs(cfg, [t], 1, dllm.Cumprod.INCLUSIVE)
        c1, c2, sd = (float(v) for v in coef[0])
        nz = dllm.randn(M * d, seed, i * M * d).reshape(M, d) if flag else 0.0
        h, h16 = x, x
        for j, W in enumerate(Wh):
            h = h @ W                                   # the reference: f32 throughout
            h16 = h16.half().float() @ W                # same with the device's f16 activations
        ref = (c1 * x + c2 * h) + sd * nz
        ref16 = (c1 * x + c2 * h16) + sd * nz
        errs.append((torch.linalg.norm(x_next - ref) / torch.linalg.norm(ref)).item())
        errs16.append((torch.linalg.norm(x_next - ref16) / torch.linalg.norm(ref16)).item())
        x = x_next
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/c5_per_step.json", "w") as f:
        json.dump({"rel_err_vs_f32_chain": errs, "rel_err_vs_f16_activation_chain": errs16,
                   "max": max(errs), "max16": max(errs16)}, f)
    print("C5 per-step max rel err vs f32 chain", max(errs), "vs f16-activation chain", max(errs16))
    assert bool(torch.isfinite(x).all())
    assert max(errs) <= 1e-3, max(errs)
