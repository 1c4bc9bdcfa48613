"""CPU suite of top-p / min-p sampling (include/dllm_quant.h, section 8k): the two restatements of the
rule (tests/token_nucleus_ref.py) agree bit for bit, the host entry point dllm_token_sample_ex_host
matches them bit for bit on tokens and {m, Z, p_token, tau}, with both masks off the outputs are
dllm_token_sample_host's, ties, constant rows, the integer boundary of the nucleus, the order of
top-k and top-p, the two ends of min-p and the degenerate rows behave as the header says, the draws
follow the masked softmax, the C entry points reject what the header says they reject, in its
order, before any device work, and the host code runs as a stand-alone program under the
sanitizers.  No GPU work here."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import token_nucleus_ref as nr
from tests import token_ref as ref
from tests import token_sample_ref as sr
from tests.host_check import run_host_check
from tests.test_token_sample_cpu import VS, known_row, rows, same
from tests.test_token_sample_cpu import host as host3

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
CHUNK = ref.CHUNK
SEED, OFFSET = 1234, 4096
PRED1 = np.nextafter(f32(1), f32(0))

TS = [1.0, 0.7]
KS = [0, 50]
TOP_PS = [2.0 ** -30, 0.1, 0.5, 0.9, 0.95, PRED1, 1.0]
MIN_PS = [0.0, 2.0 ** -33, 0.05, 0.5, 1.0]


def host(L, x, dtype=0, ld=None, T=1.0, k=0, top_p=1.0, min_p=0.0, seed=SEED, offset=OFFSET, u=None):
    """dllm_token_sample_ex_host on rows of x placed at stride ld (padding NaN / +inf); the buffer ends
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
    st = np.full((M, 4), 77, f32)
    if u is not None:
        u = np.ascontiguousarray(np.asarray(u, f32).reshape(M, 3))
    rc = L.dllm_token_sample_ex_host(buf.ctypes.data, dtype, M, V, ld, T, k, top_p, min_p,
                                     None if u is None else u.ctypes.data, seed, offset, tok.ctypes.data, st.ctypes.data)
    assert rc == 0, L.dllm_last_error()
    return tok, st


@functools.lru_cache(maxsize=None)
def prepared(V, T, k):
    """The parts of the two restatements that do not depend on top_p and min_p, for rows(V)."""
    x = rows(V)
    return [nr.Prepared(r, T, k) for r in x], [nr.PreparedLoop(r, T, k) for r in x]


@functools.lru_cache(maxsize=None)
def picked(V, T, b, tau_bits):
    """(m, Z, token, p_token) of row b of rows(V) masked at the threshold with these bits, drawn at
    counter OFFSET + b: from the vectorised sampler, and for row 0 checked against the loop form."""
    t = np.array([tau_bits], np.uint32).view(f32)[0]
    y = nr.mask(rows(V)[b], T, t)
    r = sr.Row(y)
    tok, p = sr.pick(r, sr.uniforms(SEED, OFFSET + b, 1))
    if b == 0:
        ltok, lst = sr.row_loop([f32(v) for v in y], 1.0, 0, sr.uniforms_loop(SEED, OFFSET))
        assert ltok == tok[0] and same(np.array(lst, f32), np.array([r.m, r.Z, p[0]], f32))
    return r.m, r.Z, tok[0], p[0]


def expected(V, T, k, top_p, min_p):
    """tokens [3], stats [3, 4] of rows(V); the two restatements' thresholds are compared on the way."""
    vec, loop = prepared(V, T, k)
    tok, st = np.zeros(3, np.int32), np.zeros((3, 4), f32)
    for b in range(3):
        t, tl = vec[b].tau(top_p, min_p), loop[b].tau(top_p, min_p)
        assert same(t, tl), (V, T, k, top_p, min_p, b, t, tl)
        m, Z, token, p = picked(V, T, b, int(ref.bits(t)[0]))
        tok[b], st[b] = token, (m, Z, p, t)
    return tok, st


# ---- the restatements and the host entry point, over the grid ---------------------------------------------

@pytest.mark.parametrize("V", VS)
def test_restatements_and_host_agree(dllm, V):
    L = dllm._lib.load()
    x = rows(V)
    kept = set()
    for T in TS:
        for k in KS:
            for top_p in TOP_PS:
                for min_p in MIN_PS:
                    tok, st = expected(V, T, k, top_p, min_p)
                    for dtype in (0, 1):
                        htok, hst = host(L, x, dtype, V + 3 + 2 * dtype, T, k, top_p, min_p)
                        assert same(htok, tok) and same(hst, st), (T, k, top_p, min_p, dtype, htok, tok, hst, st)
                    kept.add(int((nr.tempered(x[0], T) >= st[0, 3]).sum()))
            tok, st = expected(V, T, k, 0.9, 0.05)
            assert all(same(a, b) for a, b in zip(host(L, x, 0, V, T, k, 0.9, 0.05), (tok, st)))   # a dense ld
            ltok, lst = nr.sample_loop(x[:1], T, k, 0.9, 0.05, SEED, OFFSET)                         # end to end
            assert same(ltok, tok[:1]) and same(lst, st[:1])
            vtok, vst = nr.sample(x, T, k, 0.9, 0.05, SEED, OFFSET)
            assert same(vtok, tok) and same(vst, st)
    if V > 1000:
        assert len(kept) > 5                                   # the grid reaches many different nuclei


def test_host_f32_values_beyond_f16(dllm):
    """f32 logits that are no f16 values: products x r and differences y - m that round."""
    L = dllm._lib.load()
    x = (np.random.default_rng(5).standard_normal((3, 20001)) * 2).astype(f32)
    for T, k, top_p, min_p in ((0.7, 0, 0.9, 0.0), (1.3, 40, 0.8, 0.01), (1.0, 0, 1.0, 0.1)):
        want = nr.sample(x, T, k, top_p, min_p, 9, 2 ** 40)
        got = host(L, x, 0, 20004, T, k, top_p, min_p, 9, 2 ** 40)
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert same(nr.sample_loop(x[:1], T, k, top_p, min_p, 9, 2 ** 40)[1], want[1][:1])


# ---- named cases --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 1025, 16385, 50257])
def test_masks_off_is_token_sample(dllm, V):
    """top_p = 1 and min_p = 0: tokens and {m, Z, p_token} are dllm_token_sample_host's bits; tau is
    the top-k threshold, -inf without one."""
    L = dllm._lib.load()
    x = rows(V)
    for T, k in ((1.0, 0), (0.7, 0), (0.7, 50), (0.5, V + 7)):
        tok3, st3 = host3(L, x, 0, V + 3, T, k)
        for dtype in (0, 1):
            tok, st = host(L, x, dtype, V + 1, T, k)
            assert same(tok, tok3) and same(st[:, :3], st3)
            y = nr.tempered(x, T)
            want = np.sort(y, axis=1)[:, V - k] + f32(0) if 0 < k < V else np.full(3, -INF)
            assert same(st[:, 3], want)


def keeps(x, T, k, top_p, min_p):
    """The indices the restatement keeps of one row, and its threshold."""
    t = nr.tau(x, T, k, top_p, min_p)
    assert same(t, nr.tau_loop(x, T, k, top_p, min_p))
    return set(np.flatnonzero(nr.tempered(x, T) >= t)), t


def both(L, x, T=1.0, k=0, top_p=1.0, min_p=0.0, u=None, dtype=0):
    """The restatement's (tokens, stats) of rows x, checked equal to the host's."""
    x = np.asarray(x, f32)
    want = nr.sample(x, T, k, top_p, min_p, SEED, OFFSET, u=u)
    got = host(L, x, dtype, x.shape[1] + 2, T, k, top_p, min_p, u=u)
    assert same(got[0], want[0]) and same(got[1], want[1]), (got, want)
    return want


def test_a_constant_row_keeps_all(dllm):
    L = dllm._lib.load()
    for V in (9, CHUNK + 5):
        x = np.full((1, V), 0.25, f32)
        for top_p in TOP_PS:
            for min_p in MIN_PS:
                tok, st = both(L, x, 2.0, 3, top_p, min_p)
                assert st[0, 1] == V and 0 <= tok[0] < V                     # Z counts the kept elements
                if top_p != 1 or min_p != 0:
                    assert st[0, 3] == f32(0.125)


def test_ties_at_tau_p_across_the_chunk_edge_are_all_kept(dllm):
    L = dllm._lib.load()
    x = ref.logits(1, CHUNK + 9, seed=3)[0].copy()
    x[CHUNK - 2:CHUNK + 3] = 20.0                                            # five ties, two chunks
    x[77] = 21.0
    # the weights at T = 1: 2^32 at 21, trunc(e^-1 2^32) for each tie; the rest is below 2^-11 of that
    kept, t = keeps(x, 1.0, 0, 0.5, 0.0)
    assert t == 20 and kept == {77} | set(range(CHUNK - 2, CHUNK + 3))       # the share 0.5 ends inside the ties
    kept, t = keeps(x, 1.0, 0, 0.25, 0.0)
    assert t == 21 and kept == {77}
    n = 256
    xs = np.tile(x, (n, 1))
    tok, st = both(L, xs, 1.0, 0, 0.5, 0.0)
    assert set(tok) == {77} | set(range(CHUNK - 2, CHUNK + 3)) and {int(v) // CHUNK for v in tok} == {0, 1}
    assert (st[:, 3] == 20).all()
    z = np.where(np.arange(12) % 2 == 0, f32(0.0), f32(-0.0)).astype(f32)    # -0 equals +0, and tau is +0
    z[5] = -1.0
    tok, st = both(L, z[None], 1.0, 0, 0.5, 0.0)
    assert ref.bits(st[0, 3]) == 0 and st[0, 1] == 11


def masses(x, T, k):
    """(A_r as Python ints, r = 1 .. the number of distinct surviving values; T; those values, descending)
    of one row: A_r is the mass of everything at or above the r-th distinct value."""
    p = nr.PreparedLoop(x, T, k)
    A, out, vals = 0, [], []
    for v, w in p.pairs:
        if not w:
            break                                                            # below tau_k, or a weight of 0
        A += w
        if vals and vals[-1] == v:
            out[-1] = A
        else:
            out.append(A), vals.append(v)
    return out, p.T, vals


def neighbours(A, T):
    """The f32 neighbours of the share A / T: the largest f32 at or below it and the smallest above it
    by the integer test, and one further out each way."""
    c = f32(A / T)
    cand = sorted({float(v) for v in (np.nextafter(np.nextafter(c, f32(0)), f32(0)), np.nextafter(c, f32(0)), c,
                                      np.nextafter(c, f32(2)), np.nextafter(np.nextafter(c, f32(2)), f32(2)))})
    return [f32(v) for v in cand if 0 < v <= 1]


BOUNDARY = [(1025, 1025, 1, 1.0, 0), (32773, 32823, 2, 0.7, 0), (32773, 32823, 2, 0.5, 50), (16385, 32773, 6, 1.0, 0)]


@pytest.mark.parametrize("V,s,scale,T,k", BOUNDARY)
def test_the_integer_boundary(dllm, V, s, scale, T, k):
    """top_p just below and just above the prefix mass A_r / T at the r = 1st, 2nd, 3rd and 50th survivor
    (counted in distinct values, ties taken whole): with floor(top_p 2^32) T <= A_r 2^32 the threshold is the r-th value, else the next one;
    the host agrees with the integer rule at every neighbour."""
    L = dllm._lib.load()
    x = known_row(V, s, scale)
    A, Tt, ys = masses(x, T, k)
    assert A[-1] == Tt
    srt = np.sort(nr.tempered(x, T))[::-1]
    place = lambda r: int(np.flatnonzero(np.array(ys, f32) == srt[r - 1])[0]) + 1   # the r-th survivor's distinct value
    seen = set()
    rs = sorted({place(r) for r in (1, 2, 3, 50)})
    for r in rs:
        for top_p in neighbours(A[r - 1], Tt):
            if top_p == 1:
                continue
            P = nr.pfix(top_p)
            want = next(ys[i] for i in range(len(ys)) if A[i] * 2 ** 32 >= P * Tt)      # Python ints
            t = nr.tau(x, T, k, top_p, 0.0)
            assert same(t, f32(want + f32(0))) and same(t, nr.tau_loop(x, T, k, top_p, 0.0))
            tok, st = host(L, x[None], 0, V + 1, T, k, top_p, 0.0)
            assert same(st[0, 3], t), (r, top_p, st[0, 3], t)
            seen.add((r, int((np.array(ys, f32) >= t).sum())))
    for r in rs:                                                             # both sides of every boundary were hit
        sides = {r} if A[r - 1] == Tt else {r, r + 1}                        # the last survivor has no far side
        assert {n for rr, n in seen if rr == r} >= sides, (r, seen)


def test_top_p_is_taken_over_the_top_k_survivors(dllm):
    """One large value, 49 middling ones, and a long flat tail that carries most of the row's mass.
    Over the 50 survivors of top-k the share 0.9 ends among the middling ones; over the whole row it
    would end in the tail."""
    L = dllm._lib.load()
    V = 4000
    x = np.full(V, 0.0, f32)
    x[:50] = 4.0 - 0.01 * np.arange(50)
    x[7] = 5.0
    x = x[np.random.default_rng(1).permutation(V)].astype(f32)
    t_seq = nr.tau(x, 1.0, 50, 0.9, 0.0)
    t_row = nr.tau(x, 1.0, 0, 0.9, 0.0)
    assert t_row == 0 and t_seq > 3.5 and nr.tau(x, 1.0, 50, 1.0, 0.0) > 3.5
    tok, st = both(L, np.tile(x, (64, 1)), 1.0, 50, 0.9, 0.0)
    assert (st[:, 3] == t_seq).all() and (x[tok] >= t_seq).all()
    kept = int((x >= t_seq).sum())
    assert kept < 50 and st[0, 1] < 50                                      # fewer than top-k alone keeps


def test_the_two_ends_of_min_p(dllm):
    L = dllm._lib.load()
    x = known_row(32773, 32823, 2).copy()
    x[[5, CHUNK + 5]] = x.max()                                              # three maxima, two chunks
    for T in TS:
        y = nr.tempered(x, T)
        W, m = nr.weights(y, -INF)
        kept, t = keeps(x, T, 0, 1.0, 1.0)                                   # min_p = 1: the ties with the maximum
        assert kept == set(np.flatnonzero(y == y.max())) and len(kept) == 3 and t == m
        tok, st = both(L, np.tile(x, (32, 1)), T, 0, 1.0, 1.0)
        assert set(tok) <= kept and st[0, 1] == 3 and same(st[:, 2], np.full(32, f32(1) / f32(3)))
    x = known_row(32773, 32773, 6)                                           # a wide row: some weights are 0
    for T in (1.0, 0.7):
        y = nr.tempered(x, T)
        W, m = nr.weights(y, -INF)
        assert 0 < (W == 0).sum() < x.size
        kept, t = keeps(x, T, 0, 1.0, 2.0 ** -33)                            # mfix = 1: exactly the W = 0 leave
        assert nr.mfix(2.0 ** -33) == 1 and kept == set(np.flatnonzero(W > 0))
        tok, st = both(L, x[None], T, 0, 1.0, 2.0 ** -33)
        assert same(st[0, 3], t)


def test_min_p_is_a_threshold_where_exp_steps_down(dllm):
    """EXP is not monotone everywhere (DESIGN.md names the places): at d = -0x1.ffff74p-3 it is one ulp
    below its value at the float before.  With mfix between the two weights, the lower element
    qualifies, the upper one does not, and the threshold keeps both: the rule is the threshold."""
    L = dllm._lib.load()
    a = f32(float.fromhex("-0x1.ffff74p-3"))
    b = np.nextafter(a, -INF)
    ga, gb = ref.exp32(np.array([a, b], f32))
    assert b < a and gb > ga and float(ga).hex() == "0x1.8ebf140000000p-1"
    x = np.array([[-3.0, a, 0.0, b, -2.0]], f32)
    W, _ = nr.weights(x[0], -INF)
    assert nr.mfix(gb) == int(W[3]) > int(W[1])
    tok, st = both(L, np.tile(x, (64, 1)), 1.0, 0, 1.0, gb)
    assert same(st[0, 3], b) and set(tok) == {1, 2, 3}


def degenerate(V):
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
    for T, k, top_p, min_p in ((0.5, 0, 0.9, 0.0), (0.5, 3, 0.5, 0.05), (0.5, 0, 1.0, 0.5)):
        tok, st = both(L, x, T, k, top_p, min_p)
        for i, name in enumerate(names):
            if name == "clean":
                assert tok[i] >= 0 and np.isfinite(st[i]).all() and st[i, 1] >= 1, (i, T, k)
                assert same(st[i, [0, 1, 3]], st[0, [0, 1, 3]])             # a neighbour moves nothing
            else:
                assert tok[i] == -1 and (ref.bits(st[i]) == 0x7fc00000).all(), (name, T, k)
    keep = [i for i, n in enumerate(names) if n != "x r overflows"]       # f16: 3e38 is +inf there
    both(L, x[keep], 0.5, 3, 0.5, 0.05, dtype=1)


# ---- the rule is a sampler ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,s,scale,T,k,top_p,min_p", [(32773, 32773, 2, 0.7, 0, 0.9, 0.02),
                                                        (32773, 32823, 2, 0.7, 50, 0.9, 0.0),
                                                        (1025, 1025, 1, 1.0, 0, 0.3, 0.0),
                                                        (32773, 32773, 2, 1.0, 0, 1.0, 0.05)])
def test_the_rule_samples_the_masked_softmax(dllm, V, s, scale, T, k, top_p, min_p):
    """N = 20000 draws (seed 1234, counters 4096 ...) of one row against the f64 softmax of the masked
    y: Pearson's statistic as in the sampler's suite, |z| < 4, on rows where the reference keeps
    between 5 and 200 tokens."""
    N = 20000
    x = known_row(V, s, scale)
    r, t = nr.row(x, T, k, top_p, min_p)
    kept = int((nr.tempered(x, T) >= t).sum())
    assert 5 <= kept <= 200, kept
    tok, _ = sr.pick(r, sr.uniforms(SEED, OFFSET, N))
    assert (tok >= 0).all() and (nr.tempered(x, T)[tok] >= t).all()
    chi2, dof, z = sr.chi2_z(np.bincount(tok, minlength=V), nr.softmax_masked_f64(x, T, t))
    print(f"V {V} T {T} k {k} top_p {top_p} min_p {min_p}: kept {kept}, chi2 / dof {chi2:.1f} / {dof}, z {z:.2f}")
    assert abs(z) < 4
    L = dllm._lib.load()
    n = N if V == 1025 else 64                                               # the host draws the same tokens
    htok, hst = host(L, np.tile(x, (n, 1)), 0, None, T, k, top_p, min_p)
    assert same(htok, tok[:n]) and same(hst[:, 3], np.full(n, t))


# ---- the error contract, through the C entry points, nothing launched -------------------------------------------

def test_rejections_in_the_headers_order(dllm):
    L = dllm._lib.load()
    INV, UNS, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_UNSUPPORTED, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)       # never dereferenced: every call below returns before a launch
    W = L.dllm_token_sample_ex_workspace
    assert W(2, 40000, 0, 1.0, 0.0) == 120 and W(2, 40000, 50, 1.0, 0.0) == 128
    assert W(2, 40000, 0, 0.9, 0.0) == 128 and W(2, 40000, 0, 1.0, 0.05) == 128 and W(2, 40000, 50, 0.9, 0.05) == 128
    assert W(2, 40000, 40000, PRED1, 0.0) == 128 and W(0, 9, 3, 0.5, 0.5) == 0 and W(1, 16385, 0, 1.0, 0.0) == 40
    ws = W(2, 40000, 50, 0.9, 0.05)

    def call(logits=p, dtype=0, M=2, V=40000, ld=40000, T=1.0, k=50, top_p=0.9, min_p=0.05, u=None, tokens=p,
             stats=p, w=p, wb=ws):
        return L.dllm_token_sample_ex(logits, dtype, M, V, ld, T, k, top_p, min_p, u, 0, 0, tokens, stats, w, wb, None)

    nan, inf = float("nan"), float("inf")
    assert call(V=0, ld=0) == INV and call(ld=39999) == INV and b"ld" in L.dllm_last_error()
    assert call(V=2 ** 31, ld=2 ** 31, wb=2 ** 62) == SHAPE
    assert call(dtype=2) == UNS and call(dtype=-1) == UNS
    for T in (0.0, -1.0, nan, inf, 1e-45):
        assert call(T=T) == INV and b"temperature" in L.dllm_last_error(), T
    for top_p in (0.0, -0.5, nan, float(np.nextafter(f32(1), f32(2))), 2.0, inf):
        assert call(top_p=top_p) == INV and b"top_p" in L.dllm_last_error(), top_p
    for min_p in (-1e-30, nan, float(np.nextafter(f32(1), f32(2))), inf):
        assert call(min_p=min_p) == INV and b"min_p" in L.dllm_last_error(), min_p
    assert call(M=0) == 0 and call(M=0, logits=None, tokens=None, stats=None, w=None, wb=0) == 0
    assert call(M=0, top_p=1e-45, min_p=1.0) == 0 and call(M=0, top_p=1.0, min_p=-0.0) == 0    # the ends are valid
    for name in ("logits", "tokens", "stats", "w"):
        assert call(**{name: None}) == INV and b"NULL" in L.dllm_last_error(), name
    assert call(wb=ws - 1) == INV and b"workspace" in L.dllm_last_error()
    assert call(k=0, top_p=1.0, min_p=0.0, wb=119) == INV and call(k=0, wb=127) == INV
    assert call(w=C.c_void_p(4098)) == INV
    # the order: V / ld, V >= 2^31, the dtype, the temperature, top_p, min_p, M == 0, the pointers
    assert call(V=0, ld=0, dtype=9, T=0.0, top_p=2.0, logits=None) == INV and b"V == 0" in L.dllm_last_error()
    assert call(V=2 ** 31, ld=2 ** 31, dtype=9, T=0.0, top_p=2.0, logits=None) == SHAPE
    assert call(dtype=9, T=0.0, top_p=2.0, M=0) == UNS
    assert call(T=0.0, top_p=2.0, min_p=2.0, M=0) == INV and b"temperature" in L.dllm_last_error()
    assert call(top_p=2.0, min_p=2.0, M=0) == INV and b"top_p" in L.dllm_last_error()
    assert call(min_p=2.0, M=0) == INV and b"min_p" in L.dllm_last_error()
    assert call(min_p=2.0, logits=None) == INV and b"min_p" in L.dllm_last_error()
    assert call(M=0, wb=0) == 0

    def h(logits=p, dtype=0, M=2, V=8, ld=8, T=1.0, top_p=0.9, min_p=0.05, tokens=p, stats=p):
        return L.dllm_token_sample_ex_host(logits, dtype, M, V, ld, T, 0, top_p, min_p, None, 0, 0, tokens, stats)

    assert h(V=0) == INV and h(ld=7) == INV and h(V=2 ** 31, ld=2 ** 31) == SHAPE and h(dtype=3) == UNS
    assert h(T=0.0) == INV and h(top_p=0.0) == INV and h(top_p=nan) == INV and h(top_p=1.5) == INV
    assert h(min_p=-1.0) == INV and h(min_p=nan) == INV and h(min_p=1.5) == INV
    assert h(M=0, logits=None, tokens=None, stats=None) == 0
    assert h(logits=None) == INV and h(tokens=None) == INV and h(stats=None) == INV
    assert h(dtype=3, T=0.0, top_p=2.0, M=0) == UNS and h(T=0.0, top_p=2.0, M=0) == INV
    assert h(top_p=2.0, min_p=2.0, M=0) == INV and b"top_p" in L.dllm_last_error()
    assert h(min_p=2.0, M=0) == INV and b"min_p" in L.dllm_last_error()


def test_wrappers_exported(dllm):
    import inspect
    text = dllm._lib.HEADER.read_text()
    for sym in ("dllm_token_sample_ex_workspace", "dllm_token_sample_ex", "dllm_token_sample_ex_host"):
        assert sym in dllm._lib.SIGNATURES and sym + "(" in text and hasattr(dllm._lib.load(), sym)
    from tests.test_capi import declared_symbols
    assert set(declared_symbols()) == set(dllm._lib.SIGNATURES)
    for fn in (dllm.sample_tokens, dllm.TokenHead.sample):
        sig = inspect.signature(fn).parameters
        assert sig["top_p"].default == 1.0 and sig["min_p"].default == 0.0
    assert inspect.signature(dllm.sample_tokens).parameters["return_tau"].default is False


# ---- the stand-alone program ------------------------------------------------------------------------------------

def test_host_entry_point_under_sanitizers(tmp_path):
    """tests/cpp/token_nucleus_host_check.cpp (its own main) with csrc/host_rules.cpp and error.cpp, compiled
    by g++ under the address and undefined-behaviour sanitizers (tests/host_check.py; no hipcc, no
    library): exact-size heap buffers at every kind of V, both dtypes, padding that must not be read,
    the masks alone and together, the degenerate rows and the rejections."""
    run_host_check("token_nucleus_host_check", tmp_path)
