"""GPU suite of the token readout: dllm_token_readout bit for bit against the numpy restatement of the
rule (tests/token_ref.py; the CPU suite checks it against a second restatement and the host entry
point) at every size that reaches another path, for both dtypes, every row layout (rows that start
off 16-byte alignment, padding that must never be read, a misaligned base), the adversarial rows,
row independence, graph replay, and TokenHead end to end on a QuantLinear."""
import functools

import numpy as np
import pytest

from tests import token_ref as ref

pytestmark = pytest.mark.gpu

# V: a single element; a ragged group; one group; one full lane round from both sides and exactly;
# the chunk edge from both sides and exactly; a third, ragged chunk; the real vocabulary (four chunks).
VS = [1, 3, 4, 1023, 1024, 1025, 16383, 16384, 16385, 32773, 50257]
MS = [1, 3, 257]
DISTINCT = 16


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.int32:
        return np.array_equal(a, b)
    return np.array_equal(ref.bits(a), ref.bits(b))


def row_map(M):
    """Row r of an M-row run holds base row (5 r + 3) mod 16: the reference is computed for 16 distinct
    rows per V (a row's bits depend on the row alone), and no two rows within 16 of each other, nor
    rows r and r + 1, share their data, so a kernel that reads or writes a neighbour's row shows."""
    return (5 * np.arange(M) + 3) % DISTINCT


@functools.lru_cache(maxsize=None)
def case(V):
    """(x, tokens, stats, probs) for 16 rows of f16-valued logits (one reference serves the f32 and
    the f16 runs): computed once, never written to."""
    x = ref.logits(DISTINCT, V, seed=V)
    out = (x,) + ref.readout(x, probs=True)
    for a in out:
        a.setflags(write=False)
    return out


def place(torch, x, ld, dtype, offset=0):
    """The rows of x at stride ld inside a buffer that ends with the last row's V elements, the
    padding filled with +inf and NaN; `offset` elements in front move the base off its alignment."""
    M, V = x.shape
    buf = np.empty((M, ld), np.float32)
    buf[:, 0::2], buf[:, 1::2] = np.nan, np.inf
    buf[:, :V] = x
    flat = np.concatenate([np.full(offset, np.nan, np.float32), buf.reshape(-1)[:(M - 1) * ld + V]])
    t = torch.from_numpy(flat).cuda()
    if dtype == "f16":
        t = t.half()
    return torch.as_strided(t, (M, V), (ld, 1), offset)


def layouts(V):
    """(ld, base offset): dense rows (V odd: rows start off 16-byte alignment); ld a multiple of 4
    above V (the vector path, ragged last group, padding after every row); an odd ld with padding;
    a base one element off."""
    ld4 = (V // 4 + 2) * 4
    return [(V, 0), (ld4, 0), (ld4 + 1, 0), (ld4, 1)]


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_readout_bit_exact(dllm, cuda, V, dtype):
    import torch
    x, tok, st, p = case(V)
    for M in MS:
        rows = row_map(M)
        for ld, off in layouts(V):
            if M == 257 and (ld, off) not in layouts(V)[:2] and V > 16385:
                continue                      # the two big layouts above cover the grid at the big sizes
            lg = place(torch, x[rows], ld, dtype, off)
            gt, gs, gp = dllm.token_readout(lg, probs=True)
            assert gt.dtype == torch.int32 and tuple(gt.shape) == (M,) and tuple(gs.shape) == (M, 2)
            assert tuple(gp.shape) == (M, V) and gp.dtype == torch.float32
            what = (M, ld, off)
            assert same(gt.cpu().numpy(), tok[rows]), what
            assert same(gs.cpu().numpy(), st[rows]), what
            assert same(gp.cpu().numpy(), p[rows]), what
            gt2, gs2 = dllm.token_readout(lg)             # without probabilities: the same tokens and stats
            assert same(gt2.cpu().numpy(), tok[rows]) and same(gs2.cpu().numpy(), st[rows]), what


def test_readout_f32_values_beyond_f16(dllm, cuda):
    """f32 logits that are no f16 values (differences x - m that round), and a 1-D input."""
    import torch
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 20001)) * 2).astype(np.float32)
    tok, st, p = ref.readout(x, probs=True)
    gt, gs, gp = dllm.token_readout(torch.from_numpy(x).cuda(), probs=True)
    assert same(gt.cpu().numpy(), tok) and same(gs.cpu().numpy(), st) and same(gp.cpu().numpy(), p)
    t1, s1 = dllm.token_readout(torch.from_numpy(x[1]).cuda())
    assert int(t1) == tok[1] and same(s1.cpu().numpy(), st[1])


@functools.lru_cache(maxsize=None)
def adversarial_case(V):
    names, rows = zip(*ref.adversarial(V))
    x = np.stack(rows)
    out = (x,) + ref.readout(x, probs=True)
    for a in out:
        a.setflags(write=False)
    return (names,) + out


@pytest.mark.parametrize("V", [4, 1025, 16384, 32773, 50257])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_adversarial_rows(dllm, cuda, V, dtype):
    """Constant rows, duplicated maxima (two lanes, across a chunk edge, at 0 and V - 1), +0 against -0,
    NaNs (at 0, at V - 1, mid-chunk, at a chunk's last element with chunks after it), a chunk of -inf
    beside a finite chunk, a row of -inf, a row with +inf.  NaN rows stand between clean rows: every
    row equals the reference computed from that row alone."""
    import torch
    names, x, tok, st, p = adversarial_case(V)
    for ld, off in layouts(V)[:3]:
        gt, gs, gp = dllm.token_readout(place(torch, x, ld, dtype, off), probs=True)
        gt, gs, gp = gt.cpu().numpy(), gs.cpu().numpy(), gp.cpu().numpy()
        for i, name in enumerate(names):
            assert gt[i] == tok[i] and same(gs[i], st[i]) and same(gp[i], p[i]), (name, ld, gt[i], tok[i], gs[i], st[i])
    row = dict(zip(names, range(len(names))))
    assert gt[row["constant"]] == V - 1 and gt[row["all -inf"]] == V - 1
    assert np.isneginf(gs[row["all -inf"], 0]) and ref.bits(gs[row["all -inf"], 1]) == 0
    assert (ref.bits(gs[row["NaN at 0"]]) == 0x7fc00000).all()
    if V > ref.CHUNK:
        i = row["a chunk of -inf beside a finite chunk"]
        assert np.isfinite(gs[i]).all() and gs[i, 1] >= 1


def test_fold_examples_on_device(dllm, cuda):
    import torch
    nan, inf = float("nan"), float("inf")
    for row, want in (([9, nan, 1, 2], 3), ([9, 1, nan], 2), ([2, 2, 2], 2), ([0.0, -0.0, -1], 1), ([-inf, -inf], 1),
                      ([nan, 5, 5, 4], 2), ([7], 0), ([nan], 0)):
        for dt in (torch.float32, torch.float16):
            t, s = dllm.token_readout(torch.tensor([row], dtype=dt).cuda())
            assert int(t[0]) == want == ref.fold_token(np.array(row, np.float32)), (row, int(t[0]))


def test_nan_row_leaves_its_neighbours_alone(dllm, cuda):
    import torch
    V = 32773
    x = np.array(case(V)[0][:3])
    clean = [a.cpu().numpy() for a in dllm.token_readout(torch.from_numpy(x).cuda(), probs=True)]
    x[1, 20000] = np.nan
    got = [a.cpu().numpy() for a in dllm.token_readout(torch.from_numpy(x).cuda(), probs=True)]
    for a, b in zip(clean, got):
        assert same(a[0], b[0]) and same(a[2], b[2])
    assert (ref.bits(got[1][1]) == 0x7fc00000).all() and (ref.bits(got[2][1]) == 0x7fc00000).all()
    assert got[0][1] == ref.readout(x[1:2])[0][0]


def test_graph_replay_gives_the_same_bits(dllm, cuda):
    """Captured on its first call on the capture stream (no warm-up of that stream's workspace): no
    allocation through the C ABI, no synchronisation; the replay writes the eager call's bits."""
    import torch
    x, tok, st, p = case(50257)
    lg = torch.from_numpy(np.array(x[:3])).cuda().half()
    eager = dllm.token_readout(lg, probs=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):             # a capture stream of its own, whose workspace is new
        gt, gs, gp = dllm.token_readout(lg, probs=True)
    for _ in range(2):
        gt.zero_(), gs.zero_(), gp.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, e in zip((gt, gs, gp), eager):
            assert torch.equal(got.view(torch.int32), e.view(torch.int32))
    assert same(gt.cpu().numpy(), tok[:3]) and same(gs.cpu().numpy(), st[:3]) and same(gp.cpu().numpy(), p[:3])


@pytest.mark.parametrize("out_dtype", ["f16", "f32"])
def test_token_head_end_to_end(dllm, cuda, out_dtype):
    """TokenHead on a small head (K = 64, N = 1001, M = 5): greedy and probabilities equal
    token_readout of the layer's own output, which equals the restatement on those logits."""
    import torch
    K, N, M = 64, 1001, 5
    rng = np.random.default_rng(1)
    W = torch.from_numpy((0.5 * rng.standard_normal((K, N))).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    lin = dllm.QuantLinear.from_weight(W, b, 4, 64)
    dt = torch.float16 if out_dtype == "f16" else torch.float32
    head = dllm.TokenHead(lin, out_dtype=dt)
    assert head.vocab_size == N
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).cuda().half()
    logits = lin(x, out_dtype=dt)
    assert logits.dtype == dt and tuple(logits.shape) == (M, N)
    tok, st, p = dllm.token_readout(logits, probs=True)
    gt, pt = head.greedy(x)
    assert same(gt.cpu().numpy(), tok.cpu().numpy())
    assert same(pt.cpu().numpy(), np.float32(1.0) / st.cpu().numpy()[:, 1])
    assert same(head.probabilities(x).cpu().numpy(), p.cpu().numpy())
    rt, rs, rp = ref.readout(logits.float().cpu().numpy(), probs=True)
    assert same(tok.cpu().numpy(), rt) and same(st.cpu().numpy(), rs) and same(p.cpu().numpy(), rp)
    assert np.array_equal(rt, logits.float().cpu().numpy().argmax(axis=1))      # no ties, no NaN here
    # the greedy token's probability is the largest of its row
    assert same(pt.cpu().numpy(), p.cpu().numpy().max(axis=1))
