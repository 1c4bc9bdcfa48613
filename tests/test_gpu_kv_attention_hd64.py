"""KV attention at head dim 64 (dllm_kv_attention_hd), the head dim of the default DiffusionConfig
(hidden 768 / 12 heads): every cache width, Sq != Skv, the rescale branch, capture, and the entry
that KVCacheStore.init_kv_cache's shapes give, walked through the progressive sequence.

Bar and references as in tests/test_gpu_kv_attention_widths.py: ``REL_TOL`` relative Frobenius error
against the oracle's f64 SDPA (generic in D) on the K/V values the kernel is defined to compute with
(the oracle-dequantized codes; for the f32 state the staged values, the rule restated on the CPU).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-3  # north_star: "outputs within 1e-3 rel-err of the CPU reference"
D = 64


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
    ref = np.asarray(ref, np.float64)
    diff = float(np.linalg.norm(np.asarray(y, np.float64) - ref))
    return 0.0 if diff == 0.0 else float(diff / np.linalg.norm(ref))


def qkv(Sq, Skv, H, seed, d=D):
    """The inputs of the widths test's qkv(): Q ~ N(0,1) rounded to f16, K ~ N(0,1), V ~ 2 N(0,1) + 0.5."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((Sq, H, d)).astype(np.float32).astype(np.float16)
    K = rng.standard_normal((Skv, H, d)).astype(np.float32)
    V = (rng.standard_normal((Skv, H, d)) * 2 + 0.5).astype(np.float32)
    return Q, K, V


def oracle_deq(orc, x, bits):
    return orc.dequantize_tensor(*orc.quantize_tensor(x, bits)).reshape(x.shape)


def sdpa(orc, Q, K, V):
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
    img = np.ldexp(x.astype(np.float64), -e).astype(np.float16)
    return np.ldexp(img.astype(np.float64), e).astype(np.float32)


def quantized(dllm, torch, x, bits):
    return dllm.QuantizedTensor.quantize(dev(torch, x), bits, packed=True)


def device_kv(dllm, torch, orc, K, V, bits):
    """(K, V as the kernel takes them, K, V as it is defined to compute with) for width ``bits`` (0: f32)."""
    if bits:
        return (quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits),
                oracle_deq(orc, K, bits), oracle_deq(orc, V, bits))
    return dev(torch, K), dev(torch, V), staged(K), staged(V)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


# ---- 1: every width vs the oracle ------------------------------------------------------------------

@pytest.mark.parametrize("bits", range(0, 9))
@pytest.mark.parametrize("S,H", [(65, 3), (130, 2), (200, 2)])
def test_every_width_vs_oracle(dllm, torch, orc, S, H, bits):
    """S = 65: a one-key second block; 130 / 200: an odd (3) and an even (4) block count through the
    loop unrolled by two; H = 3: heads at odd row offsets (a row is 8 bits bytes) for the odd widths."""
    Q, K, V = qkv(S, S, H, S * 10 + H)
    kd, vd, Kh, Vh = device_kv(dllm, torch, orc, K, V, bits)
    Od = dllm.kv_attention(dev(torch, Q), kd, vd)
    assert tuple(Od.shape) == (S, H, D)
    O = host(Od.float())
    err = rel_err(O, sdpa(orc, Q, Kh, Vh))
    print(f"D 64 bits {bits} S {S} H {H}: rel_err {err:.3e}")
    assert np.isfinite(O).all()
    assert err <= REL_TOL, err


# ---- 2: the staged images pinned to the 8-bit path, bit for bit ------------------------------------

@pytest.mark.parametrize("bits", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("S,H", [(33, 2), (130, 3)])
def test_images_match_8bit_path(dllm, torch, S, H, bits):
    """The same codes and {scale, zp} repacked at 8 bits stage to the same integers, so the outputs
    are the same bytes: a wrong field extraction at D = 64's row offsets shows here."""
    Q, K, V = qkv(S, S, H, 1000 + S + H + bits)
    Qd = dev(torch, Q)
    outs = []
    for width in (bits, 8):
        kv = []
        for x in (K, V):
            t = quantized(dllm, torch, x, bits)
            if width == 8:
                t = dllm.QuantizedTensor(dllm.pack(t.codes(), 8), t.shape, t.params, 8, True)
            kv.append(t)
        outs.append(dllm.kv_attention(Qd, kv[0], kv[1]))
    assert torch.isfinite(outs[0]).all()
    assert outs[0].abs().sum().item() > 0
    assert torch.equal(outs[0], outs[1])


# ---- 3: Sq != Skv ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [2, 4, 8, 0])
@pytest.mark.parametrize("Sq,Skv", [(1, 65), (33, 130), (300, 33), (257, 64), (64, 1)])
def test_sq_differs_from_skv(dllm, torch, orc, Sq, Skv, bits):
    """Sq = 300: a second workgroup and a ragged last one; 257: one row in the second."""
    H = 2
    Q, K, V = qkv(Sq, Skv, H, 7 * Sq + Skv)
    kd, vd, Kh, Vh = device_kv(dllm, torch, orc, K, V, bits)
    Od = dllm.kv_attention(dev(torch, Q), kd, vd)
    assert tuple(Od.shape) == (Sq, H, D)
    O = host(Od.float())
    err = rel_err(O, orc.attention_rows(Q.astype(np.float32), Kh, Vh))
    print(f"D 64 bits {bits} Sq {Sq} Skv {Skv}: rel_err {err:.3e}")
    assert np.isfinite(O).all()
    assert err <= REL_TOL, err


@pytest.mark.parametrize("bits", [2, 4, 8, 0])
def test_query_rows_are_independent(dllm, torch, bits):
    """Rows 0 .. Sq-1 of the Sq = Skv = 130 call are the bytes of the call with only those queries."""
    Skv, H = 130, 2
    Q, K, V = qkv(Skv, Skv, H, 99)
    Qd = dev(torch, Q)
    kd, vd = (quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits)) if bits else (dev(torch, K), dev(torch, V))
    full = dllm.kv_attention(Qd, kd, vd)
    assert torch.isfinite(full).all()
    for Sq in (1, 33, 130):
        assert torch.equal(dllm.kv_attention(Qd[:Sq].contiguous(), kd, vd), full[:Sq]), Sq


# ---- 4: the rescale branch ---------------------------------------------------------------------------

def test_peaked_softmax(dllm, torch, orc):
    """test_kv_attention_peaked_softmax's construction at D = 64: key 200 (the 4th block) dominates
    query 5, so the running max moves late and the O tiles are rescaled."""
    S, H = 256, 1
    rng = np.random.default_rng(3)
    Q = (rng.standard_normal((S, H, D)) * 0.1).astype(np.float16)
    K = (rng.standard_normal((S, H, D)) * 0.1).astype(np.float32)
    V = rng.standard_normal((S, H, D)).astype(np.float32)
    K[200, 0, :] = 8.0 * np.sign(Q[5, 0, :].astype(np.float32))
    kq, vq = quantized(dllm, torch, K, 8), quantized(dllm, torch, V, 8)
    O = host(dllm.kv_attention(dev(torch, Q), kq, vq).float())
    Oref = orc.attention(Q.astype(np.float32), oracle_deq(orc, K, 8), oracle_deq(orc, V, 8))
    print(f"D 64 peaked: rel_err {rel_err(O, Oref):.3e}, query 5 {rel_err(O[5], Oref[5]):.3e}")
    assert np.isfinite(O).all()
    assert rel_err(O, Oref) <= REL_TOL
    assert rel_err(O[5], Oref[5]) <= REL_TOL


# ---- 5: D = 128 through the new entry point ---------------------------------------------------------

@pytest.mark.parametrize("bits", [4, 3, 0])
@pytest.mark.parametrize("S", [33, 256])
def test_d128_same_bytes_as_ex(dllm, torch, S, bits):
    H = 2
    Q, K, V = qkv(S, S, H, 5 * S + bits, d=128)
    Qd = dev(torch, Q)
    if bits:
        kq, vq = quantized(dllm, torch, K, bits), quantized(dllm, torch, V, bits)
        k, kp, v, vp = kq.data.data_ptr(), kq.params.data_ptr(), vq.data.data_ptr(), vq.params.data_ptr()
    else:
        kq, vq = dev(torch, K), dev(torch, V)
        k, kp, v, vp = kq.data_ptr(), None, vq.data_ptr(), None
    L = dllm._lib.load()
    ex, hd = (torch.zeros(S, H, 128, dtype=torch.float16, device="cuda") for _ in range(2))
    assert L.dllm_kv_attention_ex(Qd.data_ptr(), S, k, kp, v, vp, bits, S, H, 128, ex.data_ptr(), _stream(torch)) == 0
    assert L.dllm_kv_attention_hd(Qd.data_ptr(), S, k, kp, v, vp, bits, S, H, 128, hd.data_ptr(), _stream(torch)) == 0
    assert torch.isfinite(hd).all()
    assert torch.equal(ex, hd) and ex.abs().sum().item() > 0


# ---- 6: the default configuration ---------------------------------------------------------------------

def test_default_config_cache_walk(dllm, torch, orc):
    """The entry of the default DiffusionConfig's shapes (hidden 768, 12 heads: head dim 64), [layers 2,
    seq 96, hidden 768], driven through the default 50-step progressive sequence as the D = 128 cache
    walk is: at every distinct state, for both layers, entry.attention is the SDPA of the K/V that
    get_keys / get_values hand out.  Sq = 40 != seq."""
    cfg = dllm.DiffusionConfig()
    assert cfg.hidden_size == 768 and cfg.num_attention_heads == 12
    hidden, H = cfg.hidden_size, cfg.num_attention_heads
    assert hidden // H == D
    layers, seq, Sq, steps = 2, 96, 40, 50
    rng = np.random.default_rng(2024)
    K = rng.standard_normal((layers, seq, hidden)).astype(np.float32)
    V = (rng.standard_normal((layers, seq, hidden)) * 2 + 0.5).astype(np.float32)
    Q = rng.standard_normal((Sq, H, D)).astype(np.float32).astype(np.float16)
    Qd = dev(torch, Q)
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
            Od = entry.attention(Qd, layer)
            assert tuple(Od.shape) == (Sq, H, D)
            O = host(Od.float())
            assert np.isfinite(O).all()
            Kl, Vl = Kg[layer].reshape(seq, H, D), Vg[layer].reshape(seq, H, D)
            if width:
                err = rel_err(O, orc.attention_rows(Q.astype(np.float32), Kl, Vl))
                print(f"state {key} layer {layer}: rel_err {err:.3e}")
                assert err <= REL_TOL, (key, layer, err)
            else:   # the two-reference bound of test_f32_state
                O_staged = orc.attention_rows(Q.astype(np.float32), staged(Kl), staged(Vl))
                O_exact = orc.attention_rows(Q.astype(np.float32), Kl, Vl)
                e_kernel, e_round, e_total = rel_err(O, O_staged), rel_err(O_staged, O_exact), rel_err(O, O_exact)
                print(f"state {key} layer {layer}: vs staged {e_kernel:.3e}, e_round {e_round:.3e}, vs f32 {e_total:.3e}")
                assert e_kernel <= REL_TOL, (key, layer, e_kernel)
                assert e_total <= e_round + REL_TOL, (key, layer, e_total, e_round)
        seen[key] = True

    for t in range(steps - 1, -1, -1):
        is_prefill = t > steps // 2
        entry.set_phase(is_prefill)
        check_state()
        if not is_prefill:
            tb = dllm.diffusion.progressive_bits(cfg, steps, t)
            if tb != entry.decode_quant_bits:
                entry.decode_quant_bits = tb
                entry.decode_quantized = None
        entry.update(entry.keys, entry.values)
        check_state()
    assert set(seen) == {(True, 8), (False, 4), (False, 2), (False, 1), (False, 0)}, sorted(seen)


# ---- 7: capture ------------------------------------------------------------------------------------------

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


# ---- 8: argument checks ----------------------------------------------------------------------------------

def test_argument_checks(dllm, torch):
    S, H = 33, 2
    Q, K, V = qkv(S, S, H, 3)
    Qd = dev(torch, Q)
    kq, vq = quantized(dllm, torch, K, 4), quantized(dllm, torch, V, 4)
    out = torch.zeros(S, H, D, dtype=torch.float16, device="cuda")
    L, E, st = dllm._lib.load(), dllm._lib, _stream(torch)
    q, k, v, o = Qd.data_ptr(), kq.data.data_ptr(), vq.data.data_ptr(), out.data_ptr()
    kp, vp = kq.params.data_ptr(), vq.params.data_ptr()

    def hd(q_, k_, v_, o_, skv=S):
        return L.dllm_kv_attention_hd(q_, S, k_, kp, v_, vp, 4, skv, H, D, o_, st)

    for bad in ((q + 2, k, v, o), (q, k + 4, v, o), (q, k, v + 8, o), (q, k, v, o + 2)):
        assert hd(*bad) == E.ERR_INVALID_PARAMS, bad
    assert hd(q, k, v, o, skv=0) == E.ERR_INVALID_PARAMS          # softmax over no keys
    torch.cuda.synchronize()
    assert out.abs().sum().item() == 0                            # a refused call writes nothing
    assert hd(q, k, v, o) == E.OK
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, dllm.kv_attention(Qd, kq, vq))
    # the Python surface
    Q96 = torch.zeros(S, H, 96, dtype=torch.float16, device="cuda")
    K96 = torch.zeros(S, H, 96, device="cuda")
    with pytest.raises(dllm.UnsupportedOperation):
        dllm.kv_attention(Q96, K96, K96)
