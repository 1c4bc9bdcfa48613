"""GPU suite of p_losses: dllm_noise_mse bit for bit against the numpy restatement of its pinned
summation order (tests/p_losses_ref.py) at the smallest sizes that reach each part of the kernel,
the seeded-stream form against explicit noise, non-finite samples, graph capture, the workspace
check, and p_losses end to end (module function, DenoiseLoop, host entry point) on QuantLinear
layers."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import p_losses_ref as ref

pytestmark = pytest.mark.gpu

BOUND = 5.1e-6   # 85 * 2^-24 (include/dllm_quant.h)
# n: one group; lane 0's second trip; the chunk edge from both sides; a second chunk holding one
# group; several chunks + a ragged one; more than 256 chunks (the finish kernel's second trip).
BIG = 257 * 16384 + 8
SIZES = [4, 1028, 16380, 16384, 16388, 3 * 16384 + 1028, BIG]


def batch(n):
    return 2 if n == BIG else 3   # three samples show a wrong per-sample base


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(n):
    """(pred, noise, loss for f32 pred, loss for f16 pred): computed once, never written to."""
    B = batch(n)
    rng = np.random.default_rng(n)
    pred = rng.standard_normal((B, n)).astype(np.float32)
    noise = rng.standard_normal((B, n)).astype(np.float32)
    out = pred, noise, ref.noise_mse(pred, noise), ref.noise_mse(pred.astype(np.float16), noise)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_noise_mse_bit_exact(dllm, cuda, n, dtype):
    import torch
    pred, noise, want32, want16 = case(n)
    p = torch.tensor(pred).cuda()
    p, want = (p.half(), want16) if dtype == "f16" else (p, want32)
    got = dllm.noise_mse(p, torch.tensor(noise).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (batch(n),)
    got = got.cpu().numpy()
    print(n, dtype, got, want)
    assert np.array_equal(bits(got), bits(want))
    # [M, N] rows with samples = B: the same elements, the same bits
    if n % 4096 == 0 or n == 1028:
        N = 4096 if n % 4096 == 0 else 4
        got2 = dllm.noise_mse(p.reshape(-1, N), torch.tensor(noise).cuda().reshape(-1, N), samples=batch(n))
        assert np.array_equal(bits(got2.cpu().numpy()), bits(want))


@pytest.mark.parametrize("n", SIZES)
def test_noise_mse_order_patterns(dllm, cuda, n):
    """pred = 0 and noise patterns whose bits move with the order of the sum (the CPU suite shows
    which reorderings they catch): every lane of every wave distinct, per stage of the order."""
    import torch
    B = batch(n)
    runs = [("dense", 0)] if n == BIG else [(m, s) for m in ref.MASKS for s in range(3)]
    zero = torch.zeros(B, n, device="cuda")
    for mask, seed in runs:
        pat = ref.lane_pattern(B, n, seed, mask)
        got = dllm.noise_mse(zero, torch.from_numpy(pat).cuda()).cpu().numpy()
        want = ref.noise_mse(np.zeros_like(pat), pat)
        assert np.array_equal(bits(got), bits(want)), (mask, seed, got, want)


@pytest.mark.parametrize("offset", [0, 4 * 12345])
@pytest.mark.parametrize("n", [4, 1028, 16388, 3 * 16384 + 1028])
def test_stream_noise_equals_explicit(dllm, cuda, orc, n, offset):
    import torch
    pred = torch.tensor(case(n)[0]).cuda()
    B = batch(n)
    z = dllm.randn(B * n, 77, offset).reshape(B, n)
    explicit = dllm.noise_mse(pred, z).cpu().numpy()
    stream = dllm.noise_mse(pred, None, seed=77, offset=offset).cpu().numpy()
    assert np.array_equal(bits(stream), bits(explicit))
    assert np.array_equal(bits(explicit), bits(ref.noise_mse(case(n)[0], orc.randn(77, offset, B * n).reshape(B, n))))
    with pytest.raises(dllm.InvalidParams):
        dllm.noise_mse(pred, None, seed=77, offset=offset + 2)


def test_stream_is_the_one_add_noise_wrote(dllm, cuda):
    import torch
    n = 16388
    pred = torch.tensor(case(n)[0]).cuda()
    cfg = dllm.DiffusionConfig()
    x0 = torch.tensor(case(n)[1]).cuda()
    _, noise_out = dllm.add_noise(cfg, x0, [3, 500, 999], seed=9, offset=64, cumprod=dllm.Cumprod.INCLUSIVE)
    a = dllm.noise_mse(pred, None, seed=9, offset=64).cpu().numpy()
    b = dllm.noise_mse(pred, noise_out).cpu().numpy()
    assert np.array_equal(bits(a), bits(b))


def test_non_finite_samples_stay_apart(dllm, cuda):
    import torch
    n = 16388
    pred, noise = (a.copy() for a in case(n)[:2])
    pred[0, 16385] = np.nan          # in the one-group second chunk
    noise[1, 777] = np.inf
    got = dllm.noise_mse(torch.from_numpy(pred).cuda(), torch.tensor(noise).cuda()).cpu().numpy()
    assert np.isnan(got[0]) and np.isinf(got[1]) and got[1] > 0 and np.isfinite(got[2])
    assert bits(got[2]) == bits(case(n)[2][2])


def _raw(dllm, pred, noise, loss, ws, ws_bytes, seed=0, offset=0):
    import torch
    B, n = pred.shape
    return dllm._lib.load().dllm_noise_mse(C.c_void_p(pred.data_ptr()), dllm._lib.F32,
                                           None if noise is None else C.c_void_p(noise.data_ptr()), B, n, seed, offset,
                                           C.c_void_p(loss.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("n", [1028, 3 * 16384 + 1028])
def test_graph_replay_gives_the_eager_bits(dllm, cuda, n):
    """Captured on its first call on that stream (no warm-up: it never synchronises or allocates)."""
    import torch
    pred, noise, want, _ = case(n)
    p, z = torch.tensor(pred).cuda(), torch.tensor(noise).cuda()
    eager = dllm.noise_mse(p, z)
    eager_stream = dllm.noise_mse(p, None, seed=3, offset=8)
    wsb = dllm._lib.load().dllm_noise_mse_workspace(3, n)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    loss = torch.full((3,), float("nan"), device="cuda")
    loss2 = torch.full((3,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert _raw(dllm, p, z, loss, ws, wsb) == 0
            assert _raw(dllm, p, None, loss2, ws, wsb, seed=3, offset=8) == 0
        for _ in range(2):
            loss.fill_(float("nan"))
            loss2.fill_(float("nan"))
            graph.replay()
            s.synchronize()
            assert torch.equal(loss.view(torch.int32), eager.view(torch.int32))
            assert torch.equal(loss2.view(torch.int32), eager_stream.view(torch.int32))
    assert np.array_equal(bits(loss.cpu().numpy()), bits(want))


def test_short_workspace_writes_nothing(dllm, cuda):
    import torch
    n = 16388
    p, z = torch.tensor(case(n)[0]).cuda(), torch.tensor(case(n)[1]).cuda()
    wsb = dllm._lib.load().dllm_noise_mse_workspace(3, n)
    assert wsb == 3 * 2 * 4
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    loss = torch.full((3,), -7.0, device="cuda")
    assert _raw(dllm, p, z, loss, ws, wsb - 1) == dllm._lib.ERR_INVALID_PARAMS
    torch.cuda.synchronize()
    assert (loss == -7.0).all() and (ws == 0).all()
    assert _raw(dllm, p, z, loss, ws, wsb) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(loss.cpu().numpy()), bits(case(n)[2]))


# ---- end to end -----------------------------------------------------------------------------------

D_MODEL, ROWS, BATCH = 256, 8, 3
T_STEPS = [0, 500, 999]


def make_layers(dllm, torch, bits_, count):
    g = torch.Generator(device="cuda").manual_seed(100 * bits_ + count)
    return [dllm.QuantLinear.from_weight(0.08 * torch.randn(D_MODEL, D_MODEL, device="cuda", generator=g),
                                         0.1 * torch.randn(D_MODEL, device="cuda", generator=g), bits_, 128)
            for _ in range(count)]


def chain(layers, x, torch):
    h = x
    for layer in layers[:-1]:
        h = layer(h, out_dtype=torch.float16)
    return layers[-1](h, out_dtype=torch.float32)


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("bits_", [2, 4, 8])
def test_p_losses_end_to_end(dllm, cuda, bits_, count):
    import torch
    cfg = dllm.DiffusionConfig()
    layers = make_layers(dllm, torch, bits_, count)
    x = torch.from_numpy(np.random.default_rng(bits_).standard_normal((BATCH, ROWS, D_MODEL)).astype(np.float32)).cuda()
    flat = x.reshape(BATCH, ROWS * D_MODEL)
    loss, noisy, nz = dllm.p_losses(cfg, layers, x, T_STEPS, seed=5, offset=8)
    assert nz is None and noisy.shape == x.shape and tuple(loss.shape) == (BATCH,)
    # noisy: add_noise with the inclusive scan
    noisy_ref, noise_ref = dllm.add_noise(cfg, flat, T_STEPS, seed=5, offset=8, cumprod=dllm.Cumprod.INCLUSIVE)
    assert torch.equal(noisy.reshape(BATCH, -1).view(torch.int32), noisy_ref.view(torch.int32))
    # loss: the restatement on the layers' own f32 output and that noise
    eps = chain(layers, noisy_ref.reshape(BATCH * ROWS, D_MODEL), torch).reshape(BATCH, -1).cpu().numpy()
    noise_np = noise_ref.cpu().numpy()
    want = ref.noise_mse(eps, noise_np)
    got = loss.cpu().numpy()
    print(bits_, count, got, want)
    assert np.array_equal(bits(got), bits(want))
    # against the f64 MSE of the same prediction
    exact = ((noise_np.astype(np.float64) - eps.astype(np.float64)) ** 2).mean(axis=1)
    assert (np.abs(got - exact) <= BOUND * exact).all(), (got, exact)
    # explicit noise: the same bits, and the noise comes back
    loss2, noisy2, nz2 = dllm.p_losses(cfg, layers, x, T_STEPS, noise=noise_ref.reshape(x.shape))
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32)) and torch.equal(noisy2, noisy)
    assert torch.equal(nz2.reshape(BATCH, -1), noise_ref)
    # a callable model
    loss3, _, _ = dllm.p_losses(cfg, lambda h: chain(layers, h, torch), x, T_STEPS, seed=5, offset=8)
    assert torch.equal(loss3.view(torch.int32), loss.view(torch.int32))
    # the loop's method: its own layers, seed and config; inclusive whatever the loop samples with
    loop = dllm.DenoiseLoop(layers, cfg, cumprod=dllm.Cumprod.EXCLUSIVE, seed=5)
    loss4, noisy4, nz4 = loop.p_losses(x, T_STEPS, offset=8)
    assert nz4 is None and torch.equal(noisy4, noisy) and torch.equal(loss4.view(torch.int32), loss.view(torch.int32))
    with pytest.raises(dllm.ShapeMismatch):
        dllm.p_losses(cfg, layers, x, T_STEPS, noise=noise_ref)              # [B, R d] against [B, R, d]
    with pytest.raises(dllm.InvalidParams):
        dllm.p_losses(cfg, layers, x, T_STEPS[:2])
    with pytest.raises(dllm.InvalidParams):
        dllm.p_losses(cfg, layers, x, [0, 1, cfg.num_timesteps])
    for layer in layers:
        layer.close()


@pytest.mark.parametrize("bits_", [2, 4, 8])
def test_p_losses_host_equals_device_path(dllm, cuda, bits_):
    import torch
    cfg = dllm.DiffusionConfig()
    layer, = make_layers(dllm, torch, bits_, 1)
    rng = np.random.default_rng(40 + bits_)
    x = rng.standard_normal((BATCH, D_MODEL)).astype(np.float32)
    nz = rng.standard_normal((BATCH, D_MODEL)).astype(np.float32)
    betas = cfg.create_beta_schedule()
    t = np.asarray(T_STEPS, np.uint64)
    L = dllm._lib.load()

    def host(noise, D=D_MODEL):
        out = np.full(BATCH, np.nan, np.float32)
        rc = L.dllm_p_losses_host(layer._h, betas.ctypes.data, betas.size, x.ctypes.data, t.ctypes.data,
                                  None if noise is None else noise.ctypes.data, 5, 8, BATCH, D, out.ctypes.data)
        return rc, out

    rc, got = host(None)
    assert rc == 0
    want, _, _ = dllm.p_losses(cfg, [layer], torch.from_numpy(x), T_STEPS, seed=5, offset=8)
    assert np.array_equal(bits(got), bits(want.cpu().numpy()))
    rc, got = host(nz)
    assert rc == 0
    want, _, _ = dllm.p_losses(cfg, [layer], torch.from_numpy(x), T_STEPS, noise=torch.from_numpy(nz))
    assert np.array_equal(bits(got), bits(want.cpu().numpy()))
    assert host(None, D=128)[0] == dllm._lib.ERR_SHAPE_MISMATCH
    t[1] = cfg.num_timesteps
    assert host(None)[0] == dllm._lib.ERR_INVALID_PARAMS
    layer.close()
