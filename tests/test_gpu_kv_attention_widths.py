"""KV attention over every state of the phase-aware cache: packed K/V of every width 1..8, the f32
"no decode copy" state (bits 0), and a block of Sq query tokens against a cache of Skv != Sq keys.

Bar: ``REL_TOL`` (north_star 1e-3) relative Frobenius error against the oracle's f64 SDPA on the
K/V values the kernel is defined to compute with (the oracle-dequantized codes; for the f32 state
the staged values RNE_f16(x 2^-e) 2^e of include/dllm_quant.h, restated here on the CPU).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3  # north_star: "outputs within 1e-3 rel-err of the CPU reference"
D = 128


@pytest.fixture(scope="module")
def torch(cuda):
    import torch as t
    return t


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def rel_err(y, ref):
    """test_gpu_parity's rel_err; an output equal to its reference has error 0 even when the reference
    is all zeros (a 1-bit V of a symmetric tensor dequantizes to all zeros: zp rounds to a code)."""
    ref = np.asarray(ref, np.float64)
    diff = float(np.linalg.norm(np.asarray(y, np.float64) - ref))
    return 0.0 if diff == 0.0 else float(diff / np.linalg.norm(ref))


def qkv(Sq, Skv, H, seed):
    """Inputs as in test_kv_attention_vs_oracle: Q ~ N(0,1) rounded to f16, K ~ N(0,1), V ~ 2 N(0,1) + 0.5."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((Sq, H, D)).astype(np.float32).astype(np.float16)
    K = rng.standard_normal((Skv, H, D)).astype(np.float32)
    V = (rng.standard_normal((Skv, H, D)) * 2 + 0.5).astype(np.float32)
    return Q, K, V


def oracle_deq(orc, x, bits):
    return orc.dequantize_tensor(*orc.quantize_tensor(x, bits)).reshape(x.shape)


def sdpa(orc, Q, K, V):
    """f64 SDPA: orc.attention for Sq == Skv, attention_rows (a query selection against all keys) otherwise."""
    if Q.shape[0] == K.shape[0]:
        return orc.attention(Q.astype(np.float32), K, V)
    return orc.attention_rows(Q.astype(np.float32), K, V)


def staged(x):
    """The f32 state's staging rule restated: amax = max |x|; e = the integer with amax 2^-e in
    [2^14, 2^15) (0 for amax == 0); the value the kernel computes with is RNE_f16(x 2^-e) 2^e."""
    amax = float(np.max(np.abs(x))) if x.size else 0.0
    e = 0
    if amax > 0:
        e = int(np.frexp(amax)[1]) - 15
        assert 2.0 ** 14 <= amax * 2.0 ** -e < 2.0 ** 15
    img = np.ldexp(x.astype(np.float64), -e).astype(np.float16)   # the scaling is exact; one RNE
    return np.ldexp(img.astype(np.float64), e).astype(np.float32)  # f16 x 2^e: exact in f32 here


def quantized(dllm, torch, x, bits):
    return dllm.QuantizedTensor.quantize(dev(torch, x), bits, packed=True)


# ---- 1: every width vs the oracle ------------------------------------------------------------------

@pytest.mark.parametrize("bits", range(1, 9))
@pytest.mark.parametrize("S,H", [(65, 3), (200, 2)])
def test_every_width_vs_oracle(dllm, torch, orc, S, H, bits):
    """S = 65: a one-key second block; H = 3: heads at odd row offsets for the odd widths."""
    Q, K, V = qkv(S, S, H, S * 10 + H)
    O = host(dllm.kv_attention(dev(torch, Q), quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits)).float())
    Oref = sdpa(orc, Q, oracle_deq(orc, K, bits), oracle_deq(orc, V, bits))
    err = rel_err(O, Oref)
    print(f"bits {bits} S {S} H {H}: rel_err {err:.3e}")
    assert np.isfinite(O).all()
    assert err <= REL_TOL, err


# ---- 2: the staged images pinned to the 8-bit path, bit for bit ------------------------------------

@pytest.mark.parametrize("bits", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("S,H", [(33, 2), (130, 3)])
def test_images_match_8bit_path(dllm, torch, S, H, bits):
    """The same codes and {scale, zp} repacked at 8 bits stage to the same integers, so the outputs
    are the same bytes: a wrong field extraction in one lane shows here while a norm bar still passes."""
    Q, K, V = qkv(S, S, H, 1000 + S + H + bits)
    Qd = dev(torch, Q)
    outs = []
    for width in (bits, 8):
        kv = []
        for x in (K, V):
            t = quantized(dllm, torch, x, bits)
            if width == 8:   # unpack, then repack at 8 with the b-bit params
                t = dllm.QuantizedTensor(dllm.pack(t.codes(), 8), t.shape, t.params, 8, True)
            kv.append(t)
        outs.append(dllm.kv_attention(Qd, kv[0], kv[1]))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


# ---- 3: Sq != Skv ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [2, 4, 8, 0])
@pytest.mark.parametrize("Sq,Skv", [(1, 65), (33, 130), (300, 33), (257, 64), (64, 1)])
def test_sq_differs_from_skv(dllm, torch, orc, Sq, Skv, bits):
    H = 2
    Q, K, V = qkv(Sq, Skv, H, 7 * Sq + Skv)
    if bits:
        kd, vd = quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits)
        Kh, Vh = oracle_deq(orc, K, bits), oracle_deq(orc, V, bits)
    else:
        kd, vd = dev(torch, K), dev(torch, V)
        Kh, Vh = staged(K), staged(V)
    O = dllm.kv_attention(dev(torch, Q), kd, vd)
    assert tuple(O.shape) == (Sq, H, D)
    err = rel_err(host(O.float()), orc.attention_rows(Q.astype(np.float32), Kh, Vh))
    print(f"bits {bits} Sq {Sq} Skv {Skv}: rel_err {err:.3e}")
    assert err <= REL_TOL, err


@pytest.mark.parametrize("bits", [2, 4, 8, 0])
def test_query_rows_are_independent(dllm, torch, bits):
    """Rows 0 .. Sq-1 of the Sq = Skv = 130 call are the bytes of the call with only those queries."""
    Skv, H = 130, 2
    Q, K, V = qkv(Skv, Skv, H, 99)
    Qd = dev(torch, Q)
    kd, vd = (quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits)) if bits else (dev(torch, K), dev(torch, V))
    full = dllm.kv_attention(Qd, kd, vd)
    for Sq in (33, 130):
        assert torch.equal(dllm.kv_attention(Qd[:Sq].contiguous(), kd, vd), full[:Sq]), Sq


# ---- 4: the legacy entry point is untouched ------------------------------------------------------------

def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("S,H", [(256, 2), (33, 2)])
def test_legacy_entry_point_same_bytes(dllm, torch, S, H, bits):
    Q, K, V = qkv(S, S, H, 5 * S + bits)
    Qd, kq, vq = dev(torch, Q), quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits)
    L = dllm._lib.load()
    old, new = (torch.zeros(S, H, D, dtype=torch.float16, device="cuda") for _ in range(2))
    assert L.dllm_kv_attention(Qd.data_ptr(), kq.data.data_ptr(), kq.params.data_ptr(), vq.data.data_ptr(),
                               vq.params.data_ptr(), bits, S, H, D, old.data_ptr(), _stream(torch)) == 0
    assert L.dllm_kv_attention_ex(Qd.data_ptr(), S, kq.data.data_ptr(), kq.params.data_ptr(), vq.data.data_ptr(),
                                  vq.params.data_ptr(), bits, S, H, D, new.data_ptr(), _stream(torch)) == 0
    assert torch.equal(old, new) and old.abs().sum().item() > 0


def test_legacy_entry_point_still_refuses_other_widths(dllm, torch):
    S, H = 33, 2
    Q, K, V = qkv(S, S, H, 11)
    Qd, kq, vq = dev(torch, Q), quantized(dllm, torch, K, 2), quantized(dllm, torch, V, 2)
    out = torch.empty(S, H, D, dtype=torch.float16, device="cuda")
    L = dllm._lib.load()
    for bits in (0, 1, 2, 3, 5, 6, 7, 9):
        rc = L.dllm_kv_attention(Qd.data_ptr(), kq.data.data_ptr(), kq.params.data_ptr(), vq.data.data_ptr(),
                                 vq.params.data_ptr(), bits, S, H, D, out.data_ptr(), _stream(torch))
        assert rc == dllm._lib.ERR_UNSUPPORTED, bits


# ---- 5: the f32 state ------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,H,kmul,vmul", [(65, 2, 1.0, 1.0), (200, 3, 1.0, 1.0), (65, 2, 1e4, 1e-3)])
def test_f32_state(dllm, torch, orc, S, H, kmul, vmul):
    """Against f64 SDPA on the staged values only the kernel's arithmetic is left: the bar of the
    quantized paths.  Against the unrounded f32 K/V the staging's own f16 rounding comes on top:
    e_round, the distance between the two f64 references, computed here from the reference alone.
    The 1e4 / 1e-3 case moves both exponents away from 0."""
    Q, K, V = qkv(S, S, H, 31 * S + H)
    K, V = (K * np.float32(kmul)).astype(np.float32), (V * np.float32(vmul)).astype(np.float32)
    O = host(dllm.kv_attention(dev(torch, Q), dev(torch, K), dev(torch, V)).float())
    O_staged, O_exact = sdpa(orc, Q, staged(K), staged(V)), sdpa(orc, Q, K, V)
    e_kernel, e_round, e_total = rel_err(O, O_staged), rel_err(O_staged, O_exact), rel_err(O, O_exact)
    print(f"f32 state S {S} H {H} x{kmul:g}/{vmul:g}: vs staged {e_kernel:.3e}, e_round {e_round:.3e}, vs f32 {e_total:.3e}")
    assert np.isfinite(O).all()
    assert e_kernel <= REL_TOL, e_kernel
    assert e_total <= e_round + REL_TOL, (e_total, e_round)


def test_f32_state_all_zero_keys(dllm, torch):
    """amax = 0 -> e = 0, an all-zero image: every score is 0 and the output is the mean of V."""
    S, H = 65, 2
    Q, _, V = qkv(S, S, H, 17)
    O = host(dllm.kv_attention(dev(torch, Q), torch.zeros(S, H, D, device="cuda"), dev(torch, V)).float())
    mean = np.broadcast_to(staged(V).astype(np.float64).mean(axis=0), (S, H, D))
    assert rel_err(O, mean) <= REL_TOL, rel_err(O, mean)


# ---- 6: the cache walk -------------------------------------------------------------------------------------

def test_cache_walk_every_state(dllm, torch, orc):
    """A [layers 2, seq 96, hidden 256] entry driven through the default 50-step progressive sequence
    as DenoiseLoop.kv_step does (phase switch, progressive decode bits, update): at every distinct
    state, for both layers, entry.attention is the SDPA of the K/V that get_keys / get_values hand
    out.  Layer 1 proves the slice offset; Sq = 40 != seq."""
    layers, seq, H, Sq, steps = 2, 96, 2, 40, 50
    rng = np.random.default_rng(2024)
    K = rng.standard_normal((layers, seq, H * D)).astype(np.float32)
    V = (rng.standard_normal((layers, seq, H * D)) * 2 + 0.5).astype(np.float32)
    Q = rng.standard_normal((Sq, H, D)).astype(np.float32).astype(np.float16)
    Qd = dev(torch, Q)
    cfg = dllm.DiffusionConfig()
    assert cfg.progressive_precision and (cfg.prefill_bits, cfg.decode_bits) == (8, 4)
    entry = dllm.KVCacheEntry(dev(torch, K), dev(torch, V), cfg.prefill_bits, cfg.decode_bits)
    seen = {}

    def check_state():
        cur = entry._current()
        width = 0 if cur is None else cur.keys.bits
        key = (entry.is_prefill_phase, width)
        if key in seen:
            return
        Kg, Vg = host(entry.get_keys()), host(entry.get_values())
        for layer in range(layers):
            O = host(entry.attention(Qd, layer).float())
            Kl, Vl = Kg[layer].reshape(seq, H, D), Vg[layer].reshape(seq, H, D)
            if width:
                err = rel_err(O, orc.attention_rows(Q.astype(np.float32), Kl, Vl))
                print(f"state {key} layer {layer}: rel_err {err:.3e}")
                assert err <= REL_TOL, (key, layer, err)
            else:   # the bound of test_f32_state; the staging exponent is that of the slice the call is given
                Ks, Vs = staged(Kl), staged(Vl)
                O_staged = orc.attention_rows(Q.astype(np.float32), Ks, Vs)
                O_exact = orc.attention_rows(Q.astype(np.float32), Kl, Vl)
                e_kernel, e_round, e_total = rel_err(O, O_staged), rel_err(O_staged, O_exact), rel_err(O, O_exact)
                print(f"state {key} layer {layer}: vs staged {e_kernel:.3e}, e_round {e_round:.3e}, vs f32 {e_total:.3e}")
                assert e_kernel <= REL_TOL, (key, layer, e_kernel)
                assert e_total <= e_round + REL_TOL, (key, layer, e_total, e_round)
        seen[key] = True

    for t in range(steps - 1, -1, -1):
        is_prefill = t > steps // 2
        entry.set_phase(is_prefill)
        check_state()                       # the decode copy at its constructed width right after the switch
        if not is_prefill:
            tb = dllm.diffusion.progressive_bits(cfg, steps, t)
            if tb != entry.decode_quant_bits:
                entry.decode_quant_bits = tb
                entry.decode_quantized = None
        entry.update(entry.keys, entry.values)
        check_state()
    assert set(seen) == {(True, 8), (False, 4), (False, 2), (False, 1), (False, 0)}, sorted(seen)


def test_entry_attention_slice_is_the_layer(dllm, torch):
    """The in-place layer slice of an odd-width copy gives the bytes of attention on that layer's
    codes copied out and repacked on their own (same codes, same params)."""
    layers, seq, H = 3, 70, 2
    rng = np.random.default_rng(5)
    K = rng.standard_normal((layers, seq, H * D)).astype(np.float32)
    V = rng.standard_normal((layers, seq, H * D)).astype(np.float32)
    Qd = dev(torch, rng.standard_normal((seq, H, D)).astype(np.float16))
    entry = dllm.KVCacheEntry(dev(torch, K), dev(torch, V), 3, 4)   # prefill copy at an odd width
    n = seq * H * D
    for layer in range(layers):
        parts = []
        for t in (entry.prefill_quantized.keys, entry.prefill_quantized.values):
            codes = t.codes()[layer * n:(layer + 1) * n].contiguous()
            parts.append(dllm.QuantizedTensor(dllm.pack(codes, 3), (seq, H, D), t.params, 3, True))
        assert torch.equal(entry.attention(Qd, layer), dllm.kv_attention(Qd, parts[0], parts[1])), layer


# ---- 7: capture ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [2, 0])
def test_capture_replays_same_bytes(dllm, torch, bits):
    """After one eager call of the shape on the stream, the same call captured replays to the same
    bytes (one stream, no parallel branches; the workspaces are already sized)."""
    S, H = 65, 2
    Q, K, V = qkv(S, S, H, 77 + bits)
    Qd = dev(torch, Q)
    kd, vd = (quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits)) if bits else (dev(torch, K), dev(torch, V))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eager = dllm.kv_attention(Qd, kd, vd)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = dllm.kv_attention(Qd, kd, vd)
        graph.replay()
        s.synchronize()
        assert torch.equal(out, eager) and torch.isfinite(out).all()
        out.zero_()
        graph.replay()
        s.synchronize()
        assert torch.equal(out, eager)


# ---- 8: argument checks ------------------------------------------------------------------------------------------

def test_argument_checks(dllm, torch):
    S, H = 33, 2
    Q, K, V = qkv(S, S, H, 3)
    Qd, Kd, Vd = dev(torch, Q), dev(torch, K), dev(torch, V)
    kq, vq = quantized(dllm, torch, K, 4), quantized(dllm, torch, V, 4)
    out = torch.zeros(S, H, D, dtype=torch.float16, device="cuda")
    L, E, st = dllm._lib.load(), dllm._lib, _stream(torch)

    def ex(q, sq, k, kp, v, vp, bits, skv, o, h=H, d=D):
        return L.dllm_kv_attention_ex(q, sq, k, kp, v, vp, bits, skv, h, d, o, st)

    q, k, v, o = Qd.data_ptr(), kq.data.data_ptr(), vq.data.data_ptr(), out.data_ptr()
    kp, vp = kq.params.data_ptr(), vq.params.data_ptr()
    assert ex(q, S, k, kp, v, vp, 9, S, o) == E.ERR_UNSUPPORTED
    assert ex(q, S, k, kp, v, vp, 4, S, o, d=64) == E.ERR_UNSUPPORTED
    assert ex(q, S, k, kp, v, vp, 4, 0, o) == E.ERR_INVALID_PARAMS          # softmax over no keys
    assert ex(q, 0, k, kp, v, vp, 4, S, o) == E.OK                          # nothing to do, nothing written
    assert ex(q, S, k, kp, v, vp, 4, S, o, h=0) == E.OK
    assert ex(q, 0, k, kp, v, vp, 4, 0, o) == E.OK
    torch.cuda.synchronize()
    assert out.abs().sum().item() == 0
    for bad in ((q + 2, k, v, o), (q, k + 4, v, o), (q, k, v + 8, o), (q, k, v, o + 2)):
        assert ex(bad[0], S, bad[1], kp, bad[2], vp, 4, S, bad[3]) == E.ERR_INVALID_PARAMS, bad
    assert ex(None, S, k, kp, v, vp, 4, S, o) == E.ERR_INVALID_PARAMS
    assert ex(q, S, k, None, v, vp, 4, S, o) == E.ERR_INVALID_PARAMS        # params are required for codes
    assert ex(q, S, Kd.data_ptr(), None, Vd.data_ptr(), None, 0, S, o) == E.OK   # ... and ignored for f32 K/V
    torch.cuda.synchronize()
    assert torch.equal(out, dllm.kv_attention(Qd, Kd, Vd))
    # the Python surface
    with pytest.raises(dllm.InvalidParams):
        dllm.kv_attention(Qd, kq, quantized(dllm, torch, V, 8))            # mixed widths
    with pytest.raises(dllm.InvalidParams):
        dllm.kv_attention(Qd, kq, Vd)                                       # mixed states
    with pytest.raises(dllm.InvalidParams):
        dllm.kv_attention(Qd, quantized(dllm, torch, K, 3), quantized(dllm, torch, V, 3), offset=8, skv=S - 1)  # 3 B in
    with pytest.raises(dllm.ShapeMismatch):
        dllm.kv_attention(Qd, kq, vq, offset=0, skv=S + 1)
