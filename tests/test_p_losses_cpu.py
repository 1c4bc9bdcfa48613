"""CPU suite of p_losses: the two restatements of dllm_noise_mse's summation order agree bit for
bit and stay inside the derived error bound; dllm_p_losses_coeffs against the oracle's inclusive
add-noise coefficients; the workspace query and every argument error, none of which needs a device."""
import ctypes as C

import numpy as np
import pytest

from tests import p_losses_ref as ref

BOUND = 5.1e-6          # 85 * 2^-24, derived in include/dllm_quant.h
SIZES = [4, 1024, 1028, 16380, 16384, 16388]
BIG = 257 * 16384 + 8   # more than 256 chunks: the finish pass's second trip


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def data(B, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n)).astype(np.float32), rng.standard_normal((B, n)).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_restatements_agree(n):
    pred, noise = data(3, n, n)
    v, l = ref.noise_mse(pred, noise), ref.noise_mse_loop(pred, noise)
    assert np.array_equal(bits(v), bits(l)), (v, l)
    pat = ref.lane_pattern(3, n, seed=n)
    zero = np.zeros_like(pat)
    assert np.array_equal(bits(ref.noise_mse(zero, pat)), bits(ref.noise_mse_loop(zero, pat)))
    h = pred.astype(np.float16)   # f16 pred widens exactly
    assert np.array_equal(bits(ref.noise_mse(h, noise)), bits(ref.noise_mse_loop(h, noise)))


def test_restatements_agree_on_finish_second_trip():
    """n = 257 * 16384 + 8: the vectorised chunk partials feed both finish passes."""
    pred, noise = data(3, BIG, 7)
    e = ref.squared_errors(pred, noise)
    P = ref.chunk_partials(e)
    assert P.shape == (3, 258)
    v = ref.finish(P, BIG)
    l = np.array([ref.finish_loop(P[b], BIG) for b in range(3)], np.float32)
    assert np.array_equal(bits(v), bits(l))
    # a few chunks of the loop against the vectorised partials: first, a middle one, the 8-element tail
    for b, c in [(0, 0), (1, 200), (2, 257)]:
        assert bits(ref.chunk_partial_loop(e[b], c)) == bits(P[b, c])
    assert np.array_equal(bits(ref.noise_mse(pred, noise)), bits(v))
    exact = ((noise.astype(np.float64) - pred.astype(np.float64)) ** 2).mean(axis=1)
    assert (np.abs(v - exact) <= BOUND * exact).all()


@pytest.mark.parametrize("n", SIZES)
def test_restatement_within_bound_of_f64_mean(n):
    pred, noise = data(3, n, 100 + n)
    for p, z in [(pred, noise), (np.zeros_like(pred), ref.lane_pattern(3, n, seed=n))]:
        exact = ((z.astype(np.float64) - p.astype(np.float64)) ** 2).mean(axis=1)
        got = ref.noise_mse(p, z)
        assert (np.abs(got - exact) <= BOUND * exact).all(), (got, exact)


def test_lane_pattern_is_order_sensitive():
    """The patterns the GPU test uses do tell orders apart.  Each other order is stated as a
    permutation of the data fed to the pinned order: the tree's levels taken 1 .. 128 instead of
    128 .. 1 (lanes bit-reversed), groups dealt to lanes in blocks of 16 instead of round-robin,
    a lane's trips reversed, the four components reversed, two lanes swapped, two chunks swapped.
    Every one changes the bits of some sample of the masked patterns (seeds 0-2, B = 3)."""
    B, C = 3, 4
    n = C * 16384
    bitrev = np.array([int(f"{j:08b}"[::-1], 2) for j in range(256)])

    def others(g):
        yield "levels", g[:, :, :, bitrev]
        yield "blocked", g.reshape(B, C, 256, 16, 4).transpose(0, 1, 3, 2, 4)
        yield "trips", g[:, :, ::-1]
        yield "components", g[..., ::-1]
        lanes = g.copy()
        lanes[:, :, :, [3, 200]] = lanes[:, :, :, [200, 3]]
        yield "two lanes", lanes
        chunks = g.copy()
        chunks[:, [0, 1]] = chunks[:, [1, 0]]
        yield "two chunks", chunks

    seen = {}
    for mask in ref.MASKS:
        for seed in range(3):
            pat = ref.lane_pattern(B, n, seed, mask)
            base = bits(ref.noise_mse(np.zeros_like(pat), pat))
            for name, other in others(pat.reshape(B, C, 16, 256, 4)):
                o = np.ascontiguousarray(other).reshape(B, n)
                seen[name] = seen.get(name, 0) + int((bits(ref.noise_mse(np.zeros_like(o), o)) != base).sum())
    assert all(seen.values()), seen


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_p_losses_coeffs_match_oracle(dllm, orc, kind):
    cfg = dllm.DiffusionConfig(num_timesteps=50, beta_schedule=dllm.BetaSchedule(kind))
    T = cfg.num_timesteps
    t = [0, 1, T - 1]
    got = dllm.p_losses_coeffs(cfg, t, 3)
    want = orc.add_noise_coeffs(cfg.create_beta_schedule(), t, inclusive=True)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got), bits(dllm.diffusion.add_noise_coeffs(cfg, t, 3, dllm.Cumprod.INCLUSIVE)))
    with pytest.raises(dllm.InvalidParams):
        dllm.p_losses_coeffs(cfg, [0, T, 1], 3)      # alpha_bars[T] panics in the reference
    with pytest.raises(dllm.InvalidParams):
        dllm.p_losses_coeffs(cfg, [0, 1], 3)         # wrong length
    assert np.array_equal(bits(dllm.p_losses_coeffs(cfg, 1, 2)), bits(want[[1, 1]]))   # scalar t


def test_noise_mse_workspace(dllm):
    L = dllm._lib.load()
    for B, n, chunks in [(1, 4, 1), (3, 16384, 1), (3, 16388, 2), (2, 257 * 16384 + 8, 258), (5, 4096 * 4096, 1024),
                         (0, 1024, 1), (4, 0, 0)]:
        assert L.dllm_noise_mse_workspace(B, n) == B * chunks * 4


def test_noise_mse_argument_errors(dllm):
    """Every check comes before the first launch: dummy pointers, no device."""
    L, E = dllm._lib.load(), dllm._lib
    ok, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)

    def call(pred=ok, dtype=E.F32, noise=ok, B=2, n=1024, offset=0, loss=ok, ws=ok, wsb=None):
        wsb = L.dllm_noise_mse_workspace(B, n) if wsb is None else wsb
        return L.dllm_noise_mse(pred, dtype, noise, B, n, 1, offset, loss, ws, wsb, None)

    assert call(dtype=2) == E.ERR_UNSUPPORTED and call(dtype=-1) == E.ERR_UNSUPPORTED
    assert call(B=0) == E.OK and call(B=0, n=0, pred=None, loss=None, ws=None, noise=None) == E.OK
    assert call(n=0) == E.ERR_INVALID_PARAMS and b"empty" in L.dllm_last_error()
    assert call(n=1022) == E.ERR_UNSUPPORTED and call(n=3) == E.ERR_UNSUPPORTED
    assert call(noise=None, offset=6) == E.ERR_INVALID_PARAMS
    for kw in ({"pred": None}, {"loss": None}, {"ws": None}, {"pred": odd}, {"noise": odd}, {"loss": odd},
               {"ws": odd}):
        assert call(**kw) == E.ERR_INVALID_PARAMS, kw
    assert call(wsb=L.dllm_noise_mse_workspace(2, 1024) - 1) == E.ERR_INVALID_PARAMS
    assert call(B=3, n=16388, wsb=3 * 2 * 4 - 1) == E.ERR_INVALID_PARAMS and b"workspace" in L.dllm_last_error()


def test_python_wrappers_are_exported(dllm):
    for name in ("p_losses", "noise_mse", "p_losses_coeffs"):
        assert name in dllm.__all__ and callable(getattr(dllm, name))
    assert callable(dllm.DenoiseLoop.p_losses)
