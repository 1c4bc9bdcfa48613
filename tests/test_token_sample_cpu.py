"""CPU suite of token sampling (include/dllm_quant.h, section 8j): the two restatements of the rule
(tests/token_sample_ref.py) agree bit for bit, the host entry point dllm_token_sample_host matches
them bit for bit on tokens and {m, Z, p_token}, known answers pin the uniforms and the draws, {m, Z}
at temperature 1 without a mask are the readout's bits, explicit uniforms reach the edges of every
level, masks and degenerate rows behave as the header says, the draws follow the masked softmax, the
C entry points reject what the header says they reject, in its order, before any device work, and
the host code runs as a stand-alone program under the sanitizers.  No GPU work here."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import token_ref as ref
from tests import token_sample_ref as sr
from tests.host_check import run_host_check

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
CHUNK = ref.CHUNK
SEED, OFFSET = 1234, 4096
U_LAST = sr.U_MAX

VS = [1, 3, 4, 1023, 1025, 16384, 16385, 32773, 50257]
TS = [1.0, 0.5, 2.0, 0.7]


def top_ks(V):
    return sorted({0, 1, 2, 50, V - 1, V, V + 7})


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.int32:
        return np.array_equal(a, b)
    return np.array_equal(ref.bits(a), ref.bits(b))


def host(L, x, dtype=0, ld=None, T=1.0, k=0, seed=SEED, offset=OFFSET, u=None):
    """dllm_token_sample_host on rows of x placed at stride ld (padding NaN / +inf); the buffer ends
    with the last row's V elements."""
    x = np.asarray(x, f32)
    M, V = x.shape
    ld = ld or V
    buf = np.empty((M, ld), f32)
    buf[:, 0::2], buf[:, 1::2] = NAN, INF
    buf[:, :V] = x
    buf = buf.reshape(-1)[:(M - 1) * ld + V]
    buf = np.ascontiguousarray(buf.astype(np.float16) if dtype == 1 else buf)
    tok = np.full(M, -7, np.int32)
    st = np.full((M, 3), 77, f32)
    if u is not None:
        u = np.ascontiguousarray(np.asarray(u, f32).reshape(M, 3))
    rc = L.dllm_token_sample_host(buf.ctypes.data, dtype, M, V, ld, T, k, None if u is None else u.ctypes.data,
                                  seed, offset, tok.ctypes.data, st.ctypes.data)
    assert rc == 0, L.dllm_last_error()
    return tok, st


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def known_row(V, s, scale):
    """The rows of the known answers: default_rng(s).standard_normal(V) * scale, as f16 values."""
    return (np.random.default_rng(s).standard_normal(V) * scale).astype(np.float16).astype(f32)


@functools.lru_cache(maxsize=None)
def rows(V):
    """Three rows of f16-valued logits at V: computed once, never written to."""
    return frozen(ref.logits(3, V, seed=V))[0]


@functools.lru_cache(maxsize=None)
def case(V, T, k):
    """(tokens, stats) of rows(V) under (T, k), rows b at counters OFFSET + b of SEED."""
    return frozen(*sr.sample(rows(V), T, k, SEED, OFFSET))


# ---- the restatements -----------------------------------------------------------------------------------

@pytest.mark.parametrize("V", VS)
def test_restatements_agree(V):
    x = rows(V)
    for T in TS:
        for k in top_ks(V):
            tok, st = case(V, T, k)
            ltok, lst = sr.sample_loop(x[:1], T, k, SEED, OFFSET)
            assert same(tok[:1], ltok) and same(st[:1], lst), (T, k, tok[0], ltok, st[0], lst)
    if V <= 4:                                   # every EXP from exact rationals too
        for k in top_ks(V):
            ltok, lst = sr.sample_loop(x, 0.7, k, SEED, OFFSET, exact_exp=True)
            assert same(case(V, 0.7, k)[0], ltok) and same(case(V, 0.7, k)[1], lst)


def test_restatements_agree_exact_exp_one_lane_round():
    x = rows(1025)[:1]
    for k in (0, 50):
        assert all(same(a, b) for a, b in zip(sr.sample(x, 0.7, k, SEED, OFFSET),
                                              sr.sample_loop(x, 0.7, k, SEED, OFFSET, exact_exp=True)))


# ---- the host entry point -----------------------------------------------------------------------------------

@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", [0, 1])
def test_host_matches_restatement(dllm, V, dtype):
    L = dllm._lib.load()
    x = rows(V)
    for T in TS:
        for k in top_ks(V):
            tok, st = case(V, T, k)
            for ld in (V, V + 3 + 2 * dtype):
                htok, hst = host(L, x, dtype, ld, T, k)
                assert same(htok, tok) and same(hst, st), (T, k, ld, htok, tok)


def test_host_f32_values_beyond_f16(dllm):
    """f32 logits that are no f16 values: products x r and differences y - m that round."""
    L = dllm._lib.load()
    x = (np.random.default_rng(5).standard_normal((3, 20001)) * 2).astype(f32)
    for T, k in ((0.7, 0), (1.3, 40)):
        tok, st = sr.sample(x, T, k, 9, 2 ** 40)
        htok, hst = host(L, x, 0, 20004, T, k, 9, 2 ** 40)
        assert same(htok, tok) and same(hst, st)


# ---- known answers ---------------------------------------------------------------------------------------------

UNIFORMS = [(1234, 0, (0x3f5115a1, 0x3ea5f8f8, 0x3f47f33f)),
            (0, 0, (0x3f044515, 0x3f708d6e, 0x3d719c00)),
            (0xDEADBEEF12345678, 2 ** 64 - 1, (0x3f6d7fb9, 0x3d4fea10, 0x3e4e4584)),
            (7, 2 ** 32 - 1, (0x3f099bbe, 0x3f7936ac, 0x3cc01140)),
            (7, 2 ** 32, (0x3ae98200, 0x3f10e06f, 0x3e1d6830))]

DRAWS = [(1025, 1025, 1, 1.0, 0, [941, 717, 607, 218, 440, 19, 509, 516], 0x4045c000, 0x429799b4),
         (32773, 32823, 2, 0.5, 50, [19213, 15080, 20990, 16635, 28976, 15497, 17757, 1624], 0x416fe000, 0x41181f96),
         (32773, 32823, 2, 0.7, 0, [32667, 14029, 29184, 24782, 17757, 13326, 31156, 1548], 0x412b56dc, 0x4216e683)]


def test_known_uniforms():
    for seed, i, want in UNIFORMS:
        assert tuple(ref.bits(sr.uniforms(seed, i, 1))[0]) == want
        assert tuple(ref.bits(np.array(sr.uniforms_loop(seed, i), f32))) == want
    assert float(sr.recip(0.7)).hex() == "0x1.6db6dc0000000p+0"
    u = sr.uniforms(1234, 0, 4096)
    assert u.min() >= 0 and u.max() <= U_LAST


def test_known_draws(dllm):
    L = dllm._lib.load()
    for V, s, scale, T, k, want, mb, zb in DRAWS:
        x = np.tile(known_row(V, s, scale), (8, 1))
        for tok, st in (sr.sample(x, T, k, SEED, OFFSET), host(L, x, 0, V, T, k), host(L, x, 1, V + 1, T, k)):
            assert tok.tolist() == want
            assert (ref.bits(st[:, 0]) == mb).all() and (ref.bits(st[:, 1]) == zb).all()
    # the host's own Philox: every known uniform decides a two-element row the way the restatement says
    x = np.array([[0.0, 0.0]], f32)
    for seed, i, _ in UNIFORMS:
        assert same(host(L, x, seed=seed, offset=i)[0], sr.sample(x, seed=seed, offset=i)[0])


@pytest.mark.parametrize("V", [1, 1025, 16385, 50257])
def test_m_and_Z_are_the_readouts(dllm, V):
    """temperature 1 and no mask: y == x to the bit, so {m, Z} are token_ref.readout's."""
    L = dllm._lib.load()
    _, rst = ref.readout(rows(V))
    assert same(case(V, 1.0, 0)[1][:, :2], rst)
    assert same(case(V, 1.0, V + 7)[1][:, :2], rst)
    assert same(host(L, rows(V))[1][:, :2], rst)


# ---- explicit uniforms -----------------------------------------------------------------------------------------

def both(L, x, T=1.0, k=0, u=None, **kw):
    """The restatement's (tokens, stats), checked equal to the host's and, on the first row, the loop form's."""
    tok, st = sr.sample(x, T, k, u=u, **kw)
    htok, hst = host(L, x, 0, None, T, k, u=u, **kw)
    assert same(htok, tok) and same(hst, st), (htok, tok, hst, st)
    ltok, lst = sr.sample_loop(np.asarray(x)[:1], T, k, u=None if u is None else np.asarray(u, f32).reshape(-1, 3)[:1], **kw)
    assert same(ltok, tok[:1]) and same(lst, st[:1])
    return tok, st


def test_extreme_uniforms(dllm):
    L = dllm._lib.load()
    x = known_row(32773, 32823, 2)[None]
    tok, st = both(L, x, 0.7, 0, u=[[0, 0, 0]])
    assert tok[0] == 0 and sr.Row(x[0], 0.7, 0).e[0, 0, 0, 0] > 0             # chunk 0, lane 0, its first element
    tok, st = both(L, x, 0.7, 0, u=[[U_LAST] * 3])
    assert tok[0] == 32772                                                     # the row's last element
    # zero weights in front: the first element with a non-zero weight
    y = x.copy()
    y[0, :5] = -INF
    assert both(L, y, 0.7, 0, u=[[0, 0, 0]])[0][0] == 1024                     # lane 0's next element
    y[0, :CHUNK] = -INF
    assert both(L, y, 0.7, 0, u=[[0, 0, 0]])[0][0] == CHUNK
    # out of range: no pick at the level the uniform belongs to; m and Z stay
    for bad in (1.0, NAN, 2.5):
        for lvl in range(3):
            u = [0.5, 0.5, 0.5]
            u[lvl] = bad
            tok, st = both(L, x, 0.7, 0, u=[u])
            assert tok[0] == -1 and ref.bits(st[0, 2]) == 0x7fc00000
            assert ref.bits(st[0, 0]) == 0x412b56dc and ref.bits(st[0, 1]) == 0x4216e683


def test_t_equal_to_a_fold_value_moves_on(dllm):
    """A constant row of four full chunks: every weight is 1, every fold value an integer, so
    t == F_j exactly at v = (j + 1) / n: the pick is j + 1 (strict <), and j just below."""
    L = dllm._lib.load()
    x = np.full((1, 4 * CHUNK), 1.5, f32)
    down = lambda v: np.nextafter(f32(v), f32(0))
    idx = lambda c, j, q: CHUNK * c + 4 * (256 * (q // 4) + j) + q % 4
    assert both(L, x, u=[[0.25, 0.5, 0.25]])[0][0] == idx(1, 128, 16)
    assert both(L, x, u=[[down(0.25), 0.5, 0.25]])[0][0] == idx(0, 128, 16)
    assert both(L, x, u=[[0.25, down(0.5), 0.25]])[0][0] == idx(1, 127, 16)
    assert both(L, x, u=[[0.25, 0.5, down(0.25)]])[0][0] == idx(1, 128, 15)
    tok, st = both(L, x, u=[[0.75, 255 / 256, 63 / 64]])
    assert tok[0] == 4 * CHUNK - 1 and st[0, 1] == 4 * CHUNK and st[0, 2] == f32(1) / f32(4 * CHUNK)


# ---- masks ------------------------------------------------------------------------------------------------------

def draws(L, x, T, k, n=512):
    """n seeded draws of one row: the restatement's, equal to the host's; returns tokens, stats."""
    xs = np.tile(np.asarray(x, f32), (n, 1))
    tok, st = sr.sample(xs[:1], T, k, SEED, OFFSET)
    row = sr.Row(x, T, k)
    tok, p = sr.pick(row, sr.uniforms(SEED, OFFSET, n))
    htok, hst = host(L, xs, 0, None, T, k)
    assert same(htok, tok) and same(hst[:, 2], p) and (ref.bits(hst[:, :2]) == ref.bits(st[0, :2])).all()
    return tok, hst


def test_ties_at_the_kth_place_are_all_kept(dllm):
    L = dllm._lib.load()
    x = np.full(40, -2.0, f32)
    x[[3, 9, 17, 30]] = [5.0, 4.0, 4.0, 4.0]
    tok, st = draws(L, x, 1.0, 2)
    assert set(tok) == {3, 9, 17, 30}                                          # k = 2 keeps four
    e = ref.exp32(np.array([-1.0], f32))[0]
    assert same(st[0, 1], ((f32(1) + e) + e) + e)                              # lanes 0, 2, 4, 7 through the tree
    tok, st = draws(L, x, 1.0, 1)
    assert set(tok) == {3} and st[0, 1] == 1 and (st[:, 2] == 1).all()
    tok, st = draws(L, np.full(9, 0.25, f32), 2.0, 3)                           # a constant row keeps all V
    assert set(tok) == set(range(9)) and st[0, 1] == 9
    z = np.where(np.arange(12) % 2 == 0, f32(0.0), f32(-0.0)).astype(f32)      # -0 equals +0
    z[5] = -1.0
    tok, st = draws(L, z, 1.0, 4)
    assert set(tok) == set(range(12)) - {5} and ref.bits(st[0, 0]) == 0 and st[0, 1] == 11


def test_tie_run_across_a_chunk_edge(dllm):
    L = dllm._lib.load()
    x = ref.logits(1, CHUNK + 9, seed=3)[0].copy()
    x[CHUNK - 2:CHUNK + 3] = 20.0                                              # five ties, two chunks
    x[77] = 21.0
    tok, st = draws(L, x, 0.5, 3)                                              # tau = 20: six survive
    assert set(tok) == {77} | set(range(CHUNK - 2, CHUNK + 3))
    assert {int(t) // CHUNK for t in tok} == {0, 1}


def test_top_1_is_the_maximum(dllm):
    L = dllm._lib.load()
    x = known_row(32773, 32823, 2)
    tok, st = draws(L, x, 0.7, 1, n=16)
    assert (tok == x.argmax()).all() and (x == x.max()).sum() == 1
    assert st[0, 1] == 1 and same(st[:, 2], np.full(16, f32(1) / st[0, 1]))
    x[[5, CHUNK + 5]] = x.max()                                                # three maxima, two chunks
    tok, st = draws(L, x, 0.7, 1, n=64)
    assert set(tok) == set(np.flatnonzero(x == x.max())) and st[0, 1] == 3
    assert same(st[:, 2], np.full(64, f32(1) / f32(3)))


def hits(target, S):
    """A uniform v with RN(v S) == target exactly, and RN(pred(v) S) below it."""
    v = f32(target) / f32(S)
    for _ in range(8):
        v = np.nextafter(v, f32(0))
    for _ in range(16):
        if f32(v * S) == target:
            assert f32(np.nextafter(v, f32(0)) * S) < target
            return v
        v = np.nextafter(v, f32(1))
    raise AssertionError("no uniform reaches the fold value")


def test_masked_chunks_and_lanes_are_never_chosen(dllm):
    L = dllm._lib.load()
    x = np.zeros(3 * CHUNK, f32)
    x[CHUNK:2 * CHUNK] = -INF                                                  # a chunk of -inf between finite chunks
    lane = 4 * (256 * np.arange(16)[:, None] + 7) + np.arange(4)[None, :]      # lane 7 of chunk 0 ...
    x[lane.reshape(-1)] = -INF                                                 # ... is masked
    tok, st = draws(L, x, 1.0, 0, n=2048)
    assert not ((tok >= CHUNK) & (tok < 2 * CHUNK)).any() and (tok < CHUNK).any() and (tok >= 2 * CHUNK).any()
    assert not np.isin(tok, lane).any()
    assert st[0, 1] == 2 * CHUNK - 64
    # at the edges: t == F_0 at level 1 skips the empty chunk; t == F_6 at level 2 skips the empty lane
    S0 = f32(CHUNK - 64)
    u0 = hits(S0, f32(2 * CHUNK - 64))                                         # t == F_0 == F_1 < F_2
    assert both(L, x[None], u=[[u0, 0, 0]])[0][0] == 2 * CHUNK
    assert both(L, x[None], u=[[np.nextafter(u0, f32(0)), 0, 0]])[0][0] == 0
    u1 = hits(f32(7 * 64), S0)                                                 # t == F_6 == F_7 < F_8
    assert both(L, x[None], u=[[0, u1, 0]])[0][0] == 4 * 8
    assert both(L, x[None], u=[[0, np.nextafter(u1, f32(0)), 0]])[0][0] == 4 * 6


# ---- degenerate rows --------------------------------------------------------------------------------------------

def degenerate(V):
    """(names, rows): every degenerate row stands between clean rows."""
    base = ref.logits(1, V, seed=11)[0]
    out = [("clean", base)]

    def put(name, at, v, fill=None):
        r = base.copy() if fill is None else np.full(V, fill, f32)
        if at is not None:
            r[at] = v
        out.extend([(name, r), ("clean", base)])

    put("NaN at 0", 0, NAN)
    put("NaN mid-chunk", V // 2, NAN)
    put("NaN at V-1", V - 1, NAN)
    put("a row of -inf", None, 0, fill=-INF)
    put("+inf", V // 3, INF)
    put("x r overflows", V // 5, 3e38)
    return [n for n, _ in out], np.stack([r for _, r in out])


@pytest.mark.parametrize("V", [4, 1025, 32773])
def test_degenerate_rows(dllm, V):
    L = dllm._lib.load()
    names, x = degenerate(V)
    for T, k in ((0.5, 0), (0.5, 3)):
        tok, st = sr.sample(x, T, k, SEED, OFFSET)
        htok, hst = host(L, x, 0, V + 2, T, k)
        assert same(htok, tok) and same(hst, st)
        one_tok, one_st = sr.sample(x[:1], T, k, SEED, OFFSET)
        for i, name in enumerate(names):
            if name == "clean":
                assert tok[i] >= 0 and np.isfinite(st[i]).all() and st[i, 1] >= 1, (i, T, k)
                if i == 0:
                    assert tok[0] == one_tok[0] and same(st[0], one_st[0])
            else:
                assert tok[i] == -1 and (ref.bits(st[i]) == 0x7fc00000).all(), (name, T, k)
    # f16: the same rows without the f32-only one
    keep = [i for i, n in enumerate(names) if n != "x r overflows"]
    tok, st = sr.sample(x[keep], 0.5, 3, SEED, OFFSET)
    htok, hst = host(L, x[keep], 1, V + 1, 0.5, 3)
    assert same(htok, tok) and same(hst, st)


# ---- the rule is a sampler -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,s,scale,T,k", [(32773, 32773, 6, 1.0, 0), (32773, 32823, 2, 0.5, 50),
                                            (1025, 1025, 1, 1.0, 0), (32773, 32773, 2, 1.0, 0)])
def test_the_rule_samples_the_masked_softmax(dllm, V, s, scale, T, k):
    """N = 20000 draws (seed 1234, counters 4096 ...) of one row against the f64 softmax of the masked
    y: Pearson's statistic over the bins with an expected count >= 5 (the rest merged), |z| < 4 for
    z = (chi2 - dof) / sqrt(2 dof)."""
    N = 20000
    x = known_row(V, s, scale)
    tok, _ = sr.pick(sr.Row(x, T, k), sr.uniforms(SEED, OFFSET, N))
    assert (tok >= 0).all()
    chi2, dof, z = sr.chi2_z(np.bincount(tok, minlength=V), sr.softmax_masked_f64(x, T, k))
    print(f"V {V} T {T} k {k}: chi2 / dof {chi2:.1f} / {dof}, z {z:.2f}")
    assert abs(z) < 4
    if (V, scale, k) == (32773, 2, 0):
        assert set(tok // CHUNK) == {0, 1, 2}                                  # draws from all three chunks
    if V == 1025:                                                              # the host draws the same 20000
        L = dllm._lib.load()
        htok, _ = host(L, np.tile(x, (N, 1)), 0, None, T, k)
        assert same(htok, tok)


# ---- the error contract, through the C entry points, nothing launched -------------------------------------------

def test_rejections_in_the_headers_order(dllm):
    L = dllm._lib.load()
    INV, UNS, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_UNSUPPORTED, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)       # never dereferenced: every call below returns before a launch
    W = L.dllm_token_sample_workspace
    assert W(2, 40000, 0) == 2 * 3 * 20 and W(2, 40000, 50) == 2 * 3 * 20 + 8
    assert W(2, 40000, 40000) == 120 and W(2, 40000, 39999) == 128 and W(0, 9, 3) == 0
    assert W(5, 16384, 1) == 120 and W(1, 16385, 0) == 40
    ws = W(2, 40000, 50)

    def call(logits=p, dtype=0, M=2, V=40000, ld=40000, T=1.0, k=50, u=None, tokens=p, stats=p, w=p, wb=ws):
        return L.dllm_token_sample(logits, dtype, M, V, ld, T, k, u, 0, 0, tokens, stats, w, wb, None)

    assert call(V=0, ld=0) == INV and call(ld=39999) == INV and b"ld" in L.dllm_last_error()
    assert call(V=2 ** 31, ld=2 ** 31, wb=2 ** 62) == SHAPE
    assert call(dtype=2) == UNS and call(dtype=-1) == UNS
    for T in (0.0, -1.0, float("nan"), float("inf"), 1e-45, 1e-39):            # the last two: 1 / T overflows
        assert call(T=T) == INV and b"temperature" in L.dllm_last_error(), T
    assert call(M=0) == 0 and call(M=0, logits=None, tokens=None, stats=None, w=None, wb=0) == 0
    for name in ("logits", "tokens", "stats", "w"):
        assert call(**{name: None}) == INV and b"NULL" in L.dllm_last_error(), name
    assert call(wb=ws - 1) == INV and b"workspace" in L.dllm_last_error()
    assert call(k=0, wb=119) == INV and call(k=40000, wb=119) == INV           # the unmasked size is 120
    assert call(w=C.c_void_p(4098)) == INV
    # the order: V / ld, V >= 2^31, the dtype, the temperature, M == 0, the pointers
    assert call(V=0, ld=0, dtype=9, T=0.0, logits=None) == INV
    assert call(V=2 ** 31, ld=2 ** 31 - 1) == INV
    assert call(V=2 ** 31, ld=2 ** 31, dtype=9, T=0.0, logits=None) == SHAPE
    assert call(dtype=9, T=0.0, M=0) == UNS and call(dtype=9, logits=None) == UNS
    assert call(T=0.0, M=0) == INV and call(T=0.0, logits=None) == INV and b"temperature" in L.dllm_last_error()
    assert call(M=0, wb=0) == 0
    # the host form: the same checks and codes
    def h(logits=p, dtype=0, M=2, V=8, ld=8, T=1.0, tokens=p, stats=p):
        return L.dllm_token_sample_host(logits, dtype, M, V, ld, T, 0, None, 0, 0, tokens, stats)

    assert h(V=0) == INV and h(ld=7) == INV and h(V=2 ** 31, ld=2 ** 31) == SHAPE and h(dtype=3) == UNS
    assert h(T=0.0) == INV and h(T=float("nan")) == INV and h(T=1e-45) == INV
    assert h(M=0, logits=None, tokens=None, stats=None) == 0
    assert h(logits=None) == INV and h(tokens=None) == INV and h(stats=None) == INV
    assert h(V=2 ** 31, ld=2 ** 31, dtype=3) == SHAPE and h(dtype=3, T=0.0, M=0) == UNS and h(T=0.0, M=0) == INV


def test_wrappers_exported(dllm):
    for name in ("sample_tokens", "TokenHead"):
        assert name in dllm.__all__ and callable(getattr(dllm, name))
    assert dllm.decode.sample_tokens is dllm.sample_tokens and callable(dllm.TokenHead.sample)
    text = dllm._lib.HEADER.read_text()
    for sym in ("dllm_token_sample_workspace", "dllm_token_sample", "dllm_token_sample_host"):
        assert sym in dllm._lib.SIGNATURES and sym + "(" in text and hasattr(dllm._lib.load(), sym)
    from tests.test_capi import declared_symbols
    assert set(declared_symbols()) == set(dllm._lib.SIGNATURES)


# ---- the stand-alone program ------------------------------------------------------------------------------------

def test_host_entry_point_under_sanitizers(tmp_path):
    """tests/cpp/token_sample_host_check.cpp (its own main) with csrc/host_rules.cpp and error.cpp, compiled
    by g++ under the address and undefined-behaviour sanitizers (tests/host_check.py; no hipcc, no
    library): exact-size heap buffers at every kind of V, both dtypes, padding that must not be read,
    every top_k around V, explicit and seeded uniforms, the degenerate rows and the rejections."""
    run_host_check("token_sample_host_check", tmp_path)
