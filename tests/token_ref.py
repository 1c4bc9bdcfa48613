"""Two independent numpy restatements of the token readout rule (include/dllm_quant.h, section 8h):
``readout`` is vectorised, ``readout_loop`` is written as plain loops over the elements, with the
token computed by the reference's literal sequential fold and every fused multiply-add rounded from
an exact rational.  The vectorised form emulates fmaf exactly as tests/search_ref.py does (rounding
to odd in f64); the loop form uses that module's Fraction-based fma.  Both work on f32 arrays; an f16
input is widened exactly by the caller (``astype(np.float32)``), as the kernels do."""
import numpy as np

from tests.search_ref import fma32, fma_loop

f32 = np.float32
CHUNK, LANES = 16384, 256
CUT = f32(-87.0)
LOG2E = f32(float.fromhex("0x1.715476p+0"))
LN2_HI = f32(float.fromhex("0x1.62e400p-1"))
LN2_LO = f32(float.fromhex("0x1.7f7d1cp-20"))
MAGIC = f32(float.fromhex("0x1.8p+23"))
# 1/5040, 1/720, 1/120, 1/24, 1/6, 1/2, 1, 1
COEF = [f32(float.fromhex(h)) for h in ("0x1.a01a02p-13", "0x1.6c16c2p-10", "0x1.111112p-7", "0x1.555556p-5",
                                        "0x1.555556p-3", "0x1p-1", "0x1p+0", "0x1p+0")]
EXP_ULPS = 0.9371          # csrc/token_exp.hpp kExpUlps: the measured largest error of EXP
QNAN = np.array([0x7fc00000], np.uint32).view(f32)[0]
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- vectorised ---------------------------------------------------------------------------------------

def exp32(d):
    """EXP on an f32 array (any shape)."""
    d = np.asarray(d, f32)
    nan = np.isnan(d)
    live = ~nan & (d >= CUT)
    dd = np.where(live, d, f32(0)).astype(f32)
    t = dd * LOG2E
    kf = (t + MAGIC) - MAGIC
    r = fma32(kf, -LN2_HI, dd)
    r = fma32(kf, -LN2_LO, r)
    p = np.full(dd.shape, COEF[0], f32)
    for c in COEF[1:]:
        p = fma32(p, r, c)
    scale = ((kf.astype(np.int32) + 127) << 23).astype(np.uint32).view(f32)
    out = np.where(live, p * scale, f32(0)).astype(f32)
    out[nan] = QNAN
    return out


def _tree(s):
    """[..., 256] -> [...]: s[j] = s[j] + s[j + h] for j < h, h = 128 ... 1."""
    h = LANES // 2
    while h:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def _row(x):
    """One row (f32 [V]) -> token, m, Z."""
    V = x.size
    nan_at = np.flatnonzero(np.isnan(x))
    n = int(nan_at[-1]) if nan_at.size else -1
    if n == V - 1:
        token = V - 1
    else:
        tail = x[n + 1:]
        token = n + 1 + int(np.flatnonzero(tail == tail.max())[-1])
    if n >= 0:
        return token, QNAN, QNAN
    C = -(-V // CHUNK)
    pad = np.full(C * CHUNK, -np.inf, f32)
    pad[:V] = x
    pad = pad.reshape(C, CHUNK)
    mc = pad.max(axis=1) + f32(0)                               # a zero maximum is +0
    m = mc.max()
    if np.isinf(m):
        return token, m, (f32(0) if m < 0 else QNAN)
    with np.errstate(invalid="ignore"):
        e = exp32(pad - mc[:, None])                            # padding: EXP(-inf) = +0
    e[np.isneginf(mc)] = 0                                      # a chunk of -inf: Z_c = +0
    e = e.reshape(C, CHUNK // (4 * LANES), LANES, 4)            # [chunk][trip][lane][component]
    s = np.zeros((C, LANES), f32)
    for k in range(e.shape[1]):
        for l in range(4):
            s = s + e[:, k, :, l]
    Zc = _tree(s)
    with np.errstate(invalid="ignore"):
        term = np.where(np.isneginf(mc), f32(0), Zc * exp32(mc - m)).astype(f32)
    lanes = np.zeros(LANES, f32)
    for c in range(C):
        lanes[c % LANES] = lanes[c % LANES] + term[c]
    return token, m, _tree(lanes)


def readout(x, probs=False):
    """x f32 [M, V] -> tokens int32 [M], stats f32 [M, 2] (and probs f32 [M, V])."""
    x = np.asarray(x, f32)
    M, V = x.shape
    tokens, stats = np.zeros(M, np.int32), np.zeros((M, 2), f32)
    p = np.zeros((M, V), f32) if probs else None
    for b in range(M):
        tokens[b], stats[b, 0], stats[b, 1] = _row(x[b])
        if probs:
            m, Z = stats[b]
            if np.isnan(Z) or np.isneginf(m):
                p[b] = QNAN
            else:
                p[b] = exp32(x[b] - m) / Z
    return (tokens, stats, p) if probs else (tokens, stats)


def closed_form_token(x):
    """The header's closed form on its own (readout states it too; the loop form folds instead)."""
    return _closed(np.asarray(x, f32))


def _closed(x):
    V = x.size
    nan_at = np.flatnonzero(np.isnan(x))
    n = int(nan_at[-1]) if nan_at.size else -1
    if n == V - 1:
        return V - 1
    tail = x[n + 1:]
    return n + 1 + int(np.flatnonzero(tail == tail.max())[-1])


# ---- plain loops ----------------------------------------------------------------------------------------

def exp_loop(d):
    d = f32(d)
    if d != d:
        return QNAN
    if d < CUT:
        return f32(0)
    t = f32(d * LOG2E)
    kf = f32(f32(t + MAGIC) - MAGIC)
    r = fma_loop(kf, -LN2_HI, d)
    r = fma_loop(kf, -LN2_LO, r)
    p = COEF[0]
    for c in COEF[1:]:
        p = fma_loop(p, r, c)
    return f32(p * f32(2.0 ** int(kf)))


def fold_token(x):
    """sample_token's max_by, literally (diffusion_prefill/src/lib.rs:162-174), on the logits."""
    cur = 0
    for i in range(1, len(x)):
        if not (x[cur] > x[i]):
            cur = i
    return cur


def _tree_loop(s):
    s = list(s)
    h = LANES // 2
    while h:
        for j in range(h):
            s[j] = f32(s[j] + s[j + h])
        h //= 2
    return s[0]


def row_loop(x):
    x = [f32(v) for v in x]
    V = len(x)
    token = fold_token(x)
    if any(v != v for v in x):
        return token, QNAN, QNAN
    C = -(-V // CHUNK)
    mc, Zc = [], []
    for c in range(C):
        lo, hi = c * CHUNK, min(V, (c + 1) * CHUNK)
        mm = f32(-np.inf)
        for i in range(lo, hi):
            if x[i] > mm:
                mm = x[i]
        mm = f32(mm + f32(0))
        mc.append(mm)
        if np.isinf(mm):
            Zc.append(f32(0) if mm < 0 else QNAN)
            continue
        lane = [f32(0)] * LANES
        for g in range(-(-(hi - lo) // 4)):
            for l in range(4):
                i = lo + 4 * g + l
                if i < hi:
                    lane[g % LANES] = f32(lane[g % LANES] + exp_loop(f32(x[i] - mm)))
        Zc.append(_tree_loop(lane))
    m = max(mc)
    if np.isinf(m):
        return token, m, (f32(0) if m < 0 else QNAN)
    lane = [f32(0)] * LANES
    for c in range(C):
        term = f32(0) if np.isneginf(mc[c]) else f32(Zc[c] * exp_loop(f32(mc[c] - m)))
        lane[c % LANES] = f32(lane[c % LANES] + term)
    return token, m, _tree_loop(lane)


def readout_loop(x, probs=False):
    x = np.asarray(x, f32)
    M, V = x.shape
    tokens, stats = np.zeros(M, np.int32), np.zeros((M, 2), f32)
    p = np.zeros((M, V), f32) if probs else None
    for b in range(M):
        tokens[b], stats[b, 0], stats[b, 1] = row_loop(x[b])
        if probs:
            m, Z = stats[b]
            for i in range(V):
                if Z != Z or np.isneginf(m):
                    p[b, i] = QNAN
                else:
                    with np.errstate(invalid="ignore"):
                        p[b, i] = f32(exp_loop(f32(x[b, i] - m)) / Z)
    return (tokens, stats, p) if probs else (tokens, stats)


# ---- the header's derived bound against the exact softmax ----------------------------------------------

def softmax_f64(x):
    """m, sum exp(x - m) and the softmax in f64 (rows of finite values)."""
    x = np.asarray(x, np.float64)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    S = e.sum(axis=1, keepdims=True)
    return m[:, 0], S[:, 0], e / S


def bound_Z(x):
    """Relative bound on Z per row: (D + 4 e + 81 + ceil(C / 256)) u."""
    x = np.asarray(x, np.float64)
    D = (x.max(axis=1) - x.min(axis=1))
    C = -(-x.shape[1] // CHUNK)
    return (D + 4 * EXP_ULPS + 81 + -(-C // LANES)) * U


def bound_p(x):
    """Bound on |p_i - softmax_i|, relative to softmax_i, plus the absolute 2^-127."""
    x = np.asarray(x, np.float64)
    m = x.max(axis=1, keepdims=True)
    d = m - x
    C = -(-x.shape[1] // CHUNK)
    return (d + d.max(axis=1, keepdims=True) + 6 * EXP_ULPS + 82 + -(-C // LANES)) * U


# ---- inputs ----------------------------------------------------------------------------------------------

def logits(M, V, seed=0, scale=2.0):
    """N(0, scale^2) logits rounded to f16 values, as f32: one array serves the f32 and the f16 runs."""
    rng = np.random.default_rng([seed, M, V])
    return (rng.standard_normal((M, V)) * scale).astype(np.float16).astype(f32)


INF_, NAN_ = f32(np.inf), f32(np.nan)


def adversarial(V):
    """Rows of V elements that decide ties, NaNs, zeros and infinities (a list of (name, row))."""
    base = logits(1, V, seed=7)[0]
    rows = [("random", base), ("constant", np.full(V, 1.5, np.float32)), ("all -inf", np.full(V, -INF_)),
            ("zeros", np.where(np.arange(V) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32))]

    def put(name, **at):
        r = base.copy()
        for i, v in at.items():
            r[int(i[1:]) % V] = v
        rows.append((name, r))

    put("max at 0 and V-1", **{"i0": 30.0, f"i{V - 1}": 30.0})
    put("max in two lanes", **{f"i{min(5, V - 1)}": 30.0, f"i{min(40, V - 1)}": 30.0})
    put("NaN at 0", i0=NAN_)
    put("NaN at V-1", **{f"i{V - 1}": NAN_})
    put("NaN mid", **{f"i{V // 2}": NAN_, "i0": 99.0})
    put("+inf", **{f"i{V // 3}": INF_})
    put("-0 after +0", **{"i0": 0.0, f"i{V - 1}": -0.0})
    r = np.full(V, -3.0, np.float32)
    r[0], r[V - 1] = 0.0, -0.0
    rows.append(("+0 then -0 as the maxima", r))
    if V > CHUNK:
        put("max across a chunk edge", **{f"i{CHUNK - 1}": 30.0, f"i{CHUNK}": 30.0})
        put("NaN at a chunk's last element", **{f"i{CHUNK - 1}": NAN_, "i3": 50.0})
        r = base.copy()
        r[:CHUNK] = -INF_
        rows.append(("a chunk of -inf beside a finite chunk", r))
    return rows
