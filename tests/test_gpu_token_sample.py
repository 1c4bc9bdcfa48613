"""GPU suite of token sampling: dllm_token_sample bit for bit -- tokens and {m, Z, p_token} -- against
the numpy restatement of the rule (tests/token_sample_ref.py; the CPU suite checks it against a second
restatement, the host entry point and known answers) at every size that reaches another path, for both
dtypes, every row layout of the readout's suite, with and without temperature and top-k; {m, Z} against
the readout; explicit uniforms at the edges of every level; masks, adversarial and degenerate rows;
the counter's wrap and carry; graph replay; TokenHead.sample end to end."""
import numpy as np
import pytest

from tests import token_ref as ref
from tests import token_sample_ref as sr
from tests.test_gpu_token_readout import DISTINCT, layouts, place, row_map

pytestmark = pytest.mark.gpu

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
CHUNK = ref.CHUNK
VS = [1, 3, 4, 1023, 1024, 1025, 16383, 16384, 16385, 32773, 50257]
MS = [1, 3, 257]
SEED, OFFSET = 1234, 4096
U_LAST = sr.U_MAX


def modes(V):
    return [(1.0, 0), (0.7, 0), (0.5, 50), (2.0, 1), (1.0, V - 1), (1.0, V + 7)]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.int32:
        return np.array_equal(a, b)
    return np.array_equal(ref.bits(a), ref.bits(b))


def run(dllm, logits, T=1.0, k=0, seed=SEED, offset=OFFSET, u=None):
    import torch
    if u is not None:
        u = torch.from_numpy(np.ascontiguousarray(np.asarray(u, f32).reshape(-1, 3))).cuda()
    tok, st = dllm.sample_tokens(logits, T, k, seed, offset, u)
    return tok.cpu().numpy(), st.cpu().numpy()


def on_device(dllm, x, dtype="f32", **kw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, f32)).cuda()
    return run(dllm, t.half() if dtype == "f16" else t, **kw)


def expect(rows_, idx, seed, offset, u=None):
    """The restatement for a run whose row r holds prepared row idx[r] and draws at counter offset + r."""
    M = len(idx)
    u = sr.uniforms(seed, offset, M) if u is None else np.asarray(u, f32).reshape(M, 3)
    tok, st = np.zeros(M, np.int32), np.zeros((M, 3), f32)
    for d in np.unique(idx):
        at = np.flatnonzero(idx == d)
        t, p = sr.pick(rows_[d], u[at])
        tok[at], st[at, 0], st[at, 1], st[at, 2] = t, rows_[d].m, rows_[d].Z, p
    return tok, st


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("mode", range(6))
def test_sample_bit_exact(dllm, cuda, V, mode):
    import torch
    T, k = modes(V)[mode]
    x = ref.logits(DISTINCT, V, seed=V)
    prepared = [sr.Row(r, T, k) for r in x]
    for dtype in ("f32", "f16"):
        for M in MS:
            idx = row_map(M)
            want = expect(prepared, idx, SEED, OFFSET)
            for ld, off in layouts(V):
                if M == 257 and (ld, off) not in layouts(V)[:2] and V > 16385:
                    continue                  # the two big layouts above cover the grid at the big sizes
                tok, st = run(dllm, place(torch, x[idx], ld, dtype, off), T, k)
                assert tok.dtype == np.int32 and tok.shape == (M,) and st.shape == (M, 3)
                assert same(tok, want[0]) and same(st, want[1]), (dtype, M, ld, off)
    assert (want[0] >= 0).all() and (want[0] < V).all()


@pytest.mark.parametrize("V", [1, 1025, 16385, 50257])
def test_m_and_Z_are_the_readouts(dllm, cuda, V):
    import torch
    x = torch.from_numpy(ref.logits(5, V, seed=V)).cuda()
    for lg in (x, x.half()):
        _, rst = dllm.token_readout(lg)
        for k in (0, V, V + 7):
            _, st = dllm.sample_tokens(lg, 1.0, k, SEED, OFFSET)
            assert torch.equal(st[:, :2].contiguous().view(torch.int32), rst.view(torch.int32))


def test_f32_values_beyond_f16_and_one_row(dllm, cuda):
    """f32 logits that are no f16 values (products and differences that round), and a 1-D input."""
    import torch
    x = (np.random.default_rng(5).standard_normal((3, 20001)) * 2).astype(f32)
    for T, k in ((0.7, 0), (1.3, 40)):
        want = sr.sample(x, T, k, 9, 2 ** 40)
        got = on_device(dllm, x, T=T, k=k, seed=9, offset=2 ** 40)
        assert same(got[0], want[0]) and same(got[1], want[1])
    t1, s1 = dllm.sample_tokens(torch.from_numpy(x[1]).cuda(), 1.3, 40, 9, 2 ** 40 + 1)
    assert t1.dim() == 0 and int(t1) == want[0][1] and same(s1.cpu().numpy(), want[1][1])


# ---- explicit uniforms -----------------------------------------------------------------------------------------

def test_explicit_uniforms_at_the_edges(dllm, cuda):
    x = (np.random.default_rng(32823).standard_normal(32773) * 2).astype(np.float16).astype(f32)
    y = x.copy()
    y[:5] = -INF
    z = x.copy()
    z[:CHUNK] = -INF
    down = lambda v: np.nextafter(f32(v), f32(0))
    u = [[0, 0, 0], [U_LAST] * 3, [0.5, 0.5, 1.0], [0.5, 1.0, 0.5], [1.0, 0.5, 0.5], [NAN, 0.5, 0.5], [0.5, NAN, 0.5],
         [0.5, 0.5, NAN], [2.5, 0, 0]]
    for dtype in ("f32", "f16"):
        for rows_, first in ((x, 0), (y, 1024), (z, CHUNK)):
            xs = np.tile(rows_, (len(u), 1))
            want = sr.sample(xs, 0.7, 0, u=u)
            got = on_device(dllm, xs, dtype, T=0.7, k=0, u=u)
            assert same(got[0], want[0]) and same(got[1], want[1])
            assert got[0][0] == first and got[0][1] == 32772 and (got[0][2:] == -1).all()
            assert (ref.bits(got[1][2:, 2]) == 0x7fc00000).all() and np.isfinite(got[1][:, :2]).all()
    # t == F_j exactly, at each level: a constant row of four full chunks, every fold value an integer
    c = np.full(4 * CHUNK, 1.5, f32)
    u = [[0.25, 0.5, 0.25], [down(0.25), 0.5, 0.25], [0.25, down(0.5), 0.25], [0.25, 0.5, down(0.25)],
         [0.75, 255 / 256, 63 / 64]]
    idx = lambda cc, j, q: CHUNK * cc + 4 * (256 * (q // 4) + j) + q % 4
    xs = np.tile(c, (len(u), 1))
    want = sr.sample(xs, u=u)
    for dtype in ("f32", "f16"):
        got = on_device(dllm, xs, dtype, u=u)
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert got[0].tolist() == [idx(1, 128, 16), idx(0, 128, 16), idx(1, 127, 16), idx(1, 128, 15), 4 * CHUNK - 1]


# ---- masks, adversarial and degenerate rows -----------------------------------------------------------------------

def mask_rows():
    """Rows of two chunks and a bit that decide the masks (a list of (name, row, T, k))."""
    V = 2 * CHUNK + 9
    base = ref.logits(1, V, seed=3)[0]
    out = []
    r = base.copy()
    r[[3, 9, 17, CHUNK + 30]] = [25.0, 24.0, 24.0, 24.0]
    out.append(("ties across the k-th place", r, 1.0, 2))
    r = base.copy()
    r[CHUNK - 2:CHUNK + 3] = 20.0
    r[77] = 21.0
    out.append(("a tie run across a chunk edge", r, 0.5, 3))
    r = base.copy()
    r[[5, CHUNK + 5, V - 1]] = 30.0
    out.append(("top-1 with three maxima", r, 0.7, 1))
    out.append(("top-1", base, 2.0, 1))
    r = np.zeros(V, f32)
    r[CHUNK:2 * CHUNK] = -INF
    r[(4 * (256 * np.arange(16)[:, None] + 7) + np.arange(4)[None, :]).reshape(-1)] = -INF
    out.append(("a chunk of -inf between finite chunks, a masked lane", r, 1.0, 0))
    out.append(("a constant row keeps all V", np.full(V, 0.25, f32), 2.0, 3))
    z = np.where(np.arange(V) % 2 == 0, f32(0.0), f32(-0.0)).astype(f32)
    z[5] = -1.0
    out.append(("-0 equals +0", z, 1.0, 4))
    return out


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_masks(dllm, cuda, dtype):
    n = 256
    for name, r, T, k in mask_rows():
        xs = np.tile(r, (n, 1))
        row = sr.Row(r, T, k)
        tok, p = sr.pick(row, sr.uniforms(SEED, OFFSET, n))
        got = on_device(dllm, xs, dtype, T=T, k=k)
        assert same(got[0], tok) and same(got[1][:, 2], p), name
        assert (ref.bits(got[1][:, 0]) == ref.bits(row.m)).all() and (ref.bits(got[1][:, 1]) == ref.bits(row.Z)).all(), name
        kept = set(np.flatnonzero(~np.isneginf(row.y)))
        assert set(got[0]) <= kept, name
        if name == "ties across the k-th place":
            assert set(got[0]) == {3, 9, 17, CHUNK + 30}
        if name == "a tie run across a chunk edge":
            assert set(got[0]) == {77} | set(range(CHUNK - 2, CHUNK + 3))
        if name.startswith("top-1"):
            assert set(got[0]) == set(np.flatnonzero(r == r.max())) and same(got[1][:, 2], np.full(n, f32(1) / row.Z))
        if name.startswith("a chunk of -inf"):
            assert {int(t) // CHUNK for t in got[0]} <= {0, 2} and row.Z == CHUNK - 64 + 9
            u0 = f32(CHUNK - 64) / row.Z                 # at or just past F_0 == F_1: never the empty chunk
            for v in (np.nextafter(u0, f32(0)), u0, np.nextafter(u0, f32(1))):
                edge = on_device(dllm, r[None], dtype, u=[[v, 0, 0]])
                assert same(edge[0], sr.sample(r[None], u=[[v, 0, 0]])[0]) and edge[0][0] in (0, 2 * CHUNK)
        if name.startswith("a constant"):
            assert row.Z == r.size and len(kept) == r.size


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
    if V > CHUNK:
        put("NaN at a chunk's last element", CHUNK - 1, NAN)
    put("a row of -inf", None, 0, fill=-INF)
    put("+inf", V // 3, INF)
    put("x r overflows", V // 5, 3e38)
    return [n for n, _ in out], np.stack([r for _, r in out])


@pytest.mark.parametrize("V", [4, 1025, 32773])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_degenerate_rows_between_clean_rows(dllm, cuda, V, dtype):
    import torch
    names, x = degenerate(V)
    if dtype == "f16":                                   # 3e38 is +inf there: the f32-only row leaves
        keep = [i for i, n in enumerate(names) if n != "x r overflows"]
        names, x = [names[i] for i in keep], x[keep]
    for T, k in ((0.5, 0), (0.5, 3)):
        want = sr.sample(x, T, k, SEED, OFFSET)
        for ld, off in layouts(V)[:3]:
            got = run(dllm, place(torch, x, ld, dtype, off), T, k)
            assert same(got[0], want[0]) and same(got[1], want[1]), (T, k, ld)
        for i, name in enumerate(names):
            if name == "clean":
                assert got[0][i] >= 0 and np.isfinite(got[1][i]).all() and got[1][i, 1] >= 1
            else:
                assert got[0][i] == -1 and (ref.bits(got[1][i]) == 0x7fc00000).all(), name


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_adversarial_rows_of_the_readout(dllm, cuda, dtype):
    """The readout's adversarial rows (ties, zeros, NaNs, infinities, a chunk of -inf) under a mask."""
    V = 32773
    names, rows_ = zip(*ref.adversarial(V))
    x = np.stack(rows_)
    for T, k in ((1.0, 0), (0.7, 5)):
        want = sr.sample(x, T, k, SEED, OFFSET)
        got = on_device(dllm, x, dtype, T=T, k=k)
        for i, name in enumerate(names):
            assert got[0][i] == want[0][i] and same(got[1][i], want[1][i]), (name, T, k)


# ---- the counter -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,offset", [(SEED, 2 ** 64 - 2), (SEED, 2 ** 32 - 2), (0xDEADBEEF12345678, 7), (0, 0)])
def test_counter(dllm, cuda, seed, offset):
    """offset + b wraps at 2^64 and carries into the high word; a seed with a high word; rows b of one
    call equal one-row calls at offset + b."""
    import torch
    x = ref.logits(1, 1025, seed=1025)[0]
    xs = torch.from_numpy(np.tile(x, (4, 1))).cuda()
    row = sr.Row(x, 0.7, 50)
    tok, p = sr.pick(row, sr.uniforms(seed, offset, 4))
    got = run(dllm, xs, 0.7, 50, seed, offset)
    assert same(got[0], tok) and same(got[1][:, 2], p)
    for b in range(4):
        one = run(dllm, xs[b:b + 1], 0.7, 50, seed, (offset + b) % 2 ** 64)
        assert one[0][0] == tok[b] and same(one[1][0], got[1][b])
    assert len(set(map(tuple, ref.bits(sr.uniforms(seed, offset, 4))))) == 4


# ---- graph replay, the head ---------------------------------------------------------------------------------------

def test_graph_replay_gives_the_same_bits(dllm, cuda):
    """Captured on its first call on the capture stream (no warm-up of that stream's workspace): no
    allocation through the C ABI, no synchronisation; the replay writes the eager call's bits."""
    import torch
    x = ref.logits(3, 50257, seed=50257)
    lg = torch.from_numpy(x).cuda().half()
    eager = dllm.sample_tokens(lg, 0.7, 50, SEED, OFFSET)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):             # a capture stream of its own, whose workspace is new
        gt, gs = dllm.sample_tokens(lg, 0.7, 50, SEED, OFFSET)
    for _ in range(2):
        gt.zero_(), gs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, e in zip((gt, gs), eager):
            assert torch.equal(got.view(torch.int32), e.view(torch.int32))
    want = sr.sample(x, 0.7, 50, SEED, OFFSET)
    assert same(gt.cpu().numpy(), want[0]) and same(gs.cpu().numpy(), want[1])


@pytest.mark.parametrize("out_dtype", ["f16", "f32"])
def test_token_head_sample(dllm, cuda, out_dtype):
    """TokenHead.sample on the small head of the readout's end-to-end test (K = 64, N = 1001, M = 5):
    sample_tokens of the layer's own logits, which equals the restatement; top_k = 1 is greedy there."""
    import torch
    K, N, M = 64, 1001, 5
    rng = np.random.default_rng(1)
    W = torch.from_numpy((0.5 * rng.standard_normal((K, N))).astype(f32)).cuda()
    b = torch.from_numpy(rng.standard_normal(N).astype(f32)).cuda()
    lin = dllm.QuantLinear.from_weight(W, b, 4, 64)
    dt = torch.float16 if out_dtype == "f16" else torch.float32
    head = dllm.TokenHead(lin, out_dtype=dt)
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(f32)).cuda().half()
    logits = lin(x, out_dtype=dt)
    tok, st = dllm.sample_tokens(logits, 0.7, 50, SEED, OFFSET)
    ht, hp = head.sample(x, 0.7, 50, SEED, OFFSET)
    assert same(ht.cpu().numpy(), tok.cpu().numpy()) and same(hp.cpu().numpy(), st.cpu().numpy()[:, 2])
    want = sr.sample(logits.float().cpu().numpy(), 0.7, 50, SEED, OFFSET)
    assert same(tok.cpu().numpy(), want[0]) and same(st.cpu().numpy(), want[1])
    gt, gp = head.greedy(x)
    t1, p1 = head.sample(x, 0.7, 1, SEED, OFFSET)
    assert same(t1.cpu().numpy(), gt.cpu().numpy()) and (p1 == 1).all()         # no ties in this head
    t1, p1 = head.sample(x, top_k=1)
    assert same(t1.cpu().numpy(), gt.cpu().numpy())
