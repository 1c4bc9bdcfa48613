"""Every schedule of ``DenoiseLoop.sample`` against a host recursion on the oracle, bit for bit.

The reference is not another form of the loop:

    x_{i+1} = orc.p_sample(x_i, eps_i, orc.randn(seed, i M d, M d), orc.p_sample_coeffs(betas, [t_i], inclusive),
                           add_noise = t_i > 0),        t_i = steps - 1 - i,

over x as one sample of M d elements, with the oracle's own beta schedule.  eps_i comes from the
layers' plain entry points on x_i (f16 out of the first layer, f32 out of the last), which
tests/test_gpu_linear_kernels.py checks bit for bit and which are repeatable.  A noise offset or a
timestep that every form of the loop got wrong in the same way would show here.

Set-up: d = 256, two int4 g128 layers, M = 48 (the last layer is unfused: PLAN_NOT_FUSED, p_sample
and cast kernels follow the GEMM) and M = 192 (the fused epilogue), 5 steps with beta 0.01 .. 0.2,
K/V 1 x 64 x 256 in a KVCacheEntry(8, 4).  In every schedule the cache must end in the state
``orc.KVCacheEntryRef`` reaches under ``orc.sample_kv_step``: phase, decode width, and
get_keys / get_values by bits.  Each schedule runs once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D_MODEL, STEPS, SEED = 256, 5, 3
MS = (48, 192)
PLAN_NOT_FUSED = 8


class PlainLast:
    """A last layer without forward_psample (as a tensor-parallel pair is): the loop follows it
    with DeviceLoopOps.p_sample."""

    def __init__(self, lin):
        self.lin = lin

    def __call__(self, h, out_dtype=None):
        return self.lin(h, out_dtype=out_dtype)


# id -> (overlap, noise, kv_spread, f16_handoff, last layer wrapped)
SCHEDULES = {
    "serial": (False, "epilogue", True, True, False),
    "overlap_epilogue": (True, "epilogue", True, True, False),
    "overlap_epilogue_no_kv_spread": (True, "epilogue", False, True, False),
    "overlap_side": (True, "side", True, True, False),
    "overlap_side_no_f16_handoff": (True, "side", True, False, False),
    "serial_plain_last": (False, "epilogue", True, True, True),
    "overlap_plain_last": (True, "epilogue", True, True, True),
}


@pytest.fixture(scope="module")
def world(dllm, cuda, orc):
    """Layers, inputs and, computed once, the reference's final x per M and final cache state."""
    import torch
    d = D_MODEL
    g = torch.Generator(device="cuda").manual_seed(4)
    layers = [dllm.QuantLinear.from_weight(0.04 * torch.randn(d, d, device="cuda", generator=g), None, 4, 128)
              for _ in range(2)]
    cfg = dllm.DiffusionConfig(num_timesteps=STEPS, beta_start=0.01, beta_end=0.2)
    K = torch.randn(1, 64, d, device="cuda", generator=g)
    V = torch.randn(1, 64, d, device="cuda", generator=g) * 2
    betas = orc.beta_schedule(orc.BETA_LINEAR, STEPS, 0.01, 0.2)
    x0, ref = {}, {}
    for M in MS:
        assert bool(layers[-1].plan(M, fused=True).flags & PLAN_NOT_FUSED) == (M <= 64)
        x0[M] = torch.randn(M, d, device="cuda", generator=g)
        x = x0[M].cpu().numpy()
        for i, t in enumerate(range(STEPS - 1, -1, -1)):
            h = layers[0](torch.from_numpy(x).cuda(), out_dtype=torch.float16)
            eps = layers[1](h, out_dtype=torch.float32).cpu().numpy()
            x = orc.p_sample(x.reshape(1, -1), eps.reshape(1, -1), orc.randn(SEED, i * M * d, M * d).reshape(1, -1),
                             orc.p_sample_coeffs(betas, [t], inclusive=True), add_noise=t > 0).reshape(M, d)
        assert np.isfinite(x).all()
        ref[M] = x
    kv = orc.KVCacheEntryRef(K.cpu().numpy(), V.cpu().numpy(), cfg.prefill_bits, cfg.decode_bits)
    assert (cfg.prefill_bits, cfg.decode_bits) == (8, 4)
    for t in range(STEPS - 1, -1, -1):
        orc.sample_kv_step(kv, t, STEPS, cfg.decode_bits, cfg.min_decode_bits)

    class W:
        pass
    W.torch, W.dllm, W.layers, W.cfg, W.K, W.V, W.x0, W.ref, W.kv = torch, dllm, layers, cfg, K, V, x0, ref, kv
    yield W
    for lin in layers:
        lin.close()


def make_loop(w, schedule):
    overlap, noise, kv_spread, f16_handoff, plain_last = SCHEDULES[schedule]
    layers = [w.layers[0], PlainLast(w.layers[1])] if plain_last else w.layers
    loop = w.dllm.DenoiseLoop(layers, w.cfg, cumprod=w.dllm.Cumprod.INCLUSIVE, seed=SEED, kv_cache=fresh_cache(w),
                              overlap=overlap, noise=noise)
    loop.kv_spread, loop.f16_handoff = kv_spread, f16_handoff
    assert loop.noise_mode == ("side" if plain_last else noise)
    return loop


def fresh_cache(w):
    return w.dllm.KVCacheEntry.new(w.K.clone(), w.V.clone(), 8, 4)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_run(w, loop, M):
    out = loop.sample(w.x0[M].clone(), STEPS)
    w.torch.cuda.synchronize()
    bad = np.argwhere(bits(out.cpu().numpy()) != bits(w.ref[M]))
    assert bad.size == 0, (M, len(bad), bad[:4].tolist())
    kv, ref = loop.kv_cache, w.kv
    assert kv.is_prefill_phase == ref.is_prefill_phase and kv.decode_quant_bits == ref.decode_quant_bits
    assert np.array_equal(bits(kv.get_keys().cpu().numpy()), bits(ref.get_keys()))
    assert np.array_equal(bits(kv.get_values().cpu().numpy()), bits(ref.get_values()))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_schedule_matches_host_recursion(world, schedule, M):
    check_run(world, make_loop(world, schedule), M)


@pytest.mark.parametrize("schedule", ["overlap_side", "overlap_epilogue"])
def test_second_sample_and_other_m(world, schedule):
    """A second sample() on the same loop object (it reuses the side stream and the noise buffers),
    then one at the other M (the noise buffers are reallocated), each from a fresh cache."""
    loop = make_loop(world, schedule)
    for M in (192, 192, 48, 192):
        loop.kv_cache = fresh_cache(world)
        check_run(world, loop, M)
