"""GPU suite of top-p / min-p sampling: dllm_token_sample_ex bit for bit -- tokens and {m, Z, p_token,
tau} -- against the numpy restatement of the rule (tests/token_nucleus_ref.py; the CPU suite checks
it against a second restatement and the host entry point) at every size that reaches another path,
for both dtypes, dense and padded rows off their alignment, the masks alone, together and after
top-k; the integer boundary of the nucleus; ties across a chunk edge; a constant row; degenerate rows
beside healthy ones; both masks off against dllm_token_sample; the Python defaults; graph replay."""
import functools

import numpy as np
import pytest

from tests import token_nucleus_ref as nr
from tests import token_ref as ref
from tests import token_sample_ref as sr
from tests.test_gpu_token_readout import place
from tests.test_token_nucleus_cpu import BOUNDARY, degenerate, masses, neighbours
from tests.test_token_sample_cpu import known_row

pytestmark = pytest.mark.gpu

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
CHUNK = ref.CHUNK
VS = [1, 3, 4, 1023, 1025, 16384, 16385, 32773, 50257]
SEED, OFFSET = 1234, 4096
PRED1 = np.nextafter(f32(1), f32(0))
T = 0.7
TOP_PS = [2.0 ** -30, 0.5, 0.95, PRED1]
MIN_PS = [0.0, 0.05, 1.0]
KS = [0, 50]
DISTINCT = 3


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.int32:
        return np.array_equal(a, b)
    return np.array_equal(ref.bits(a), ref.bits(b))


@functools.lru_cache(maxsize=None)
def base(V):
    x = ref.logits(DISTINCT, V, seed=V)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def prepared(V, k):
    return [nr.Prepared(r, T, k) for r in base(V)]


@functools.lru_cache(maxsize=None)
def masked_row(V, d, tau_bits):
    """token_sample_ref's prepared form of base row d masked at the threshold with these bits."""
    t = np.array([tau_bits], np.uint32).view(f32)[0]
    return sr.Row(nr.mask(base(V)[d], T, t))


def expect(V, k, top_p, min_p, idx):
    """The restatement for a run whose row r holds base row idx[r] and draws at counter OFFSET + r."""
    M = len(idx)
    u = sr.uniforms(SEED, OFFSET, M)
    tok, st = np.zeros(M, np.int32), np.zeros((M, 4), f32)
    for d in np.unique(idx):
        at = np.flatnonzero(idx == d)
        t = prepared(V, k)[d].tau(top_p, min_p)
        row = masked_row(V, int(d), int(ref.bits(t)[0]))
        tk, p = sr.pick(row, u[at])
        tok[at], st[at, 0], st[at, 1], st[at, 2], st[at, 3] = tk, row.m, row.Z, p, t
    return tok, st


def run(dllm, logits, temperature=T, k=0, top_p=1.0, min_p=0.0, u=None):
    import torch
    if u is not None:
        u = torch.from_numpy(np.ascontiguousarray(np.asarray(u, f32).reshape(-1, 3))).cuda()
    tok, st = dllm.sample_tokens(logits, temperature, k, SEED, OFFSET, u, top_p=top_p, min_p=min_p, return_tau=True)
    return tok.cpu().numpy(), st.cpu().numpy()


def on_device(dllm, x, dtype="f32", **kw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, f32)).cuda()
    return run(dllm, t.half() if dtype == "f16" else t, **kw)


@pytest.mark.parametrize("V", VS)
def test_sample_ex_bit_exact(dllm, cuda, V):
    import torch
    for M in (3, 65) if V == 1025 else (3,):             # 65 rows: more than one wave of blocks of the search
        idx = (5 * np.arange(M) + 3) % DISTINCT
        x = base(V)[idx]
        for dtype in ("f32", "f16"):
            for ld, off in ((V, 0), (V + 3, 1)):         # dense; padded with NaN / +inf, the base one element off
                lg = place(torch, x, ld, dtype, off)
                for k in KS:
                    for top_p in TOP_PS:
                        for min_p in MIN_PS:
                            want = expect(V, k, top_p, min_p, idx)
                            tok, st = run(dllm, lg, T, k, top_p, min_p)
                            assert tok.dtype == np.int32 and tok.shape == (M,) and st.shape == (M, 4)
                            assert same(tok, want[0]) and same(st, want[1]), (M, dtype, ld, k, top_p, min_p, st, want[1])
    assert (want[0] >= 0).all() and (want[0] < V).all()


def test_min_p_alone_and_one_row(dllm, cuda):
    """top_p = 1 with min_p on (the search without the histogram), f32 values that are no f16 values,
    and a 1-D input."""
    import torch
    x = (np.random.default_rng(5).standard_normal((3, 20001)) * 2).astype(f32)
    for temperature, k, top_p, min_p in ((0.7, 0, 1.0, 0.05), (1.3, 40, 1.0, 0.01), (0.7, 0, 0.9, 0.0), (1.3, 40, 0.8, 0.01)):
        want = nr.sample(x, temperature, k, top_p, min_p, SEED, OFFSET)
        got = on_device(dllm, x, temperature=temperature, k=k, top_p=top_p, min_p=min_p)
        assert same(got[0], want[0]) and same(got[1], want[1])
    t1, s1 = dllm.sample_tokens(torch.from_numpy(x[1]).cuda(), 1.3, 40, SEED, OFFSET + 1, top_p=0.8, min_p=0.01,
                                return_tau=True)
    assert t1.dim() == 0 and int(t1) == want[0][1] and same(s1.cpu().numpy(), want[1][1])


def test_the_integer_boundary(dllm, cuda):
    """The f32 neighbours of the prefix masses A_r / T (r = 1, 2, 3, 50) as top_p, at V = 16385."""
    V, s, scale, temperature, k = [c for c in BOUNDARY if c[0] == 16385][0]
    x = known_row(V, s, scale)
    A, Tt, ys = masses(x, temperature, k)
    srt = np.sort(nr.tempered(x, temperature))[::-1]
    hit = set()
    for r in (1, 2, 3, 50):
        d = int(np.flatnonzero(np.array(ys, f32) == srt[r - 1])[0])
        for top_p in neighbours(A[d], Tt):
            if top_p == 1:
                continue
            want = nr.sample(x[None], temperature, k, top_p, 0.0, SEED, OFFSET)
            for dtype in ("f32", "f16"):
                got = on_device(dllm, x[None], dtype, temperature=temperature, k=k, top_p=top_p)
                assert same(got[0], want[0]) and same(got[1], want[1]), (r, top_p, got[1], want[1])
            hit.add((r, int((srt >= want[1][0, 3]).sum())))
    assert len({n for _, n in hit}) >= 6                  # both sides of the boundaries were reached


def test_ties_across_the_chunk_edge_and_a_constant_row(dllm, cuda):
    x = ref.logits(1, CHUNK + 9, seed=3)[0].copy()
    x[CHUNK - 2:CHUNK + 3] = 20.0                         # five ties, two chunks
    x[77] = 21.0
    n = 256
    xs = np.tile(x, (n, 1))
    want = nr.sample(xs[:1], 1.0, 0, 0.5, 0.0, SEED, OFFSET)
    row, t = nr.row(x, 1.0, 0, 0.5, 0.0)
    tok, p = sr.pick(row, sr.uniforms(SEED, OFFSET, n))
    for dtype in ("f32", "f16"):
        got = on_device(dllm, xs, dtype, temperature=1.0, top_p=0.5)
        assert same(got[0], tok) and same(got[1][:, 2], p) and (ref.bits(got[1][:, [0, 1, 3]]) == ref.bits(want[1][0, [0, 1, 3]])).all()
        assert t == 20 and set(got[0]) == {77} | set(range(CHUNK - 2, CHUNK + 3))
    for V in (9, CHUNK + 5):
        c = np.full((4, V), 0.25, f32)
        for top_p, min_p in ((0.5, 0.0), (1.0, 1.0), (2.0 ** -30, 0.05), (PRED1, 0.0)):
            want = nr.sample(c, 2.0, 3, top_p, min_p, SEED, OFFSET)
            for dtype in ("f32", "f16"):
                got = on_device(dllm, c, dtype, temperature=2.0, k=3, top_p=top_p, min_p=min_p)
                assert same(got[0], want[0]) and same(got[1], want[1])
                assert (got[1][:, 1] == V).all() and (got[1][:, 3] == f32(0.125)).all()      # all V are kept


@pytest.mark.parametrize("V", [4, 1025, 32773])
def test_degenerate_rows_beside_healthy_rows(dllm, cuda, V):
    import torch
    names, x = degenerate(V)
    for dtype in ("f32", "f16"):
        nm, xs = names, x
        if dtype == "f16":                                # 3e38 is +inf there: the f32-only row leaves
            keep = [i for i, n in enumerate(names) if n != "x r overflows"]
            nm, xs = [names[i] for i in keep], x[keep]
        for k, top_p, min_p in ((0, 0.9, 0.0), (3, 0.5, 0.05), (0, 1.0, 0.5)):
            want = nr.sample(xs, 0.5, k, top_p, min_p, SEED, OFFSET)
            got = run(dllm, place(torch, xs, V + 3, dtype, 1), 0.5, k, top_p, min_p)
            assert same(got[0], want[0]) and same(got[1], want[1]), (dtype, k, top_p, min_p)
            for i, name in enumerate(nm):
                if name == "clean":
                    assert got[0][i] >= 0 and np.isfinite(got[1][i]).all() and got[1][i, 1] >= 1
                    assert same(got[1][i, [0, 1, 3]], got[1][0, [0, 1, 3]])                  # a neighbour moves nothing
                else:
                    assert got[0][i] == -1 and (ref.bits(got[1][i]) == 0x7fc00000).all(), name


@pytest.mark.parametrize("V", [1, 1025, 16385, 50257])
def test_masks_off_is_token_sample(dllm, cuda, V):
    """top_p = 1 and min_p = 0: dllm_token_sample_ex gives dllm_token_sample's bits on the device, and
    tau is the select's threshold (-inf without top-k)."""
    import torch
    x = torch.from_numpy(base(V).copy()).cuda()
    for lg in (x, x.half()):
        for temperature, k in ((1.0, 0), (0.7, 50), (0.5, V + 7)):
            tok3, st3 = dllm.sample_tokens(lg, temperature, k, SEED, OFFSET)
            tok4, st4 = dllm.sample_tokens(lg, temperature, k, SEED, OFFSET, return_tau=True)
            assert tuple(st3.shape) == (DISTINCT, 3) and tuple(st4.shape) == (DISTINCT, 4)
            assert torch.equal(tok3, tok4) and torch.equal(st4[:, :3].contiguous().view(torch.int32), st3.view(torch.int32))
            y = nr.tempered(base(V), temperature)
            want = np.sort(y, axis=1)[:, V - k] + f32(0) if 0 < k < V else np.full(DISTINCT, -INF)
            assert same(st4[:, 3].cpu().numpy(), want)


def test_python_defaults_reach_the_old_entry_point(dllm, cuda, monkeypatch):
    """sample_tokens and TokenHead.sample with the defaults: dllm_token_sample, stats [M, 3], as before;
    with a mask on: the new entry point, stats still [M, 3] unless tau is asked for."""
    import torch
    L = dllm._lib.load()
    lg = torch.from_numpy(base(1025).copy()).cuda()
    before = dllm.sample_tokens(lg, T, 50, SEED, OFFSET)
    masked = dllm.sample_tokens(lg, T, 50, SEED, OFFSET, top_p=0.5)
    assert tuple(masked[1].shape) == (DISTINCT, 3)
    want = expect(1025, 50, 0.5, 0.0, np.arange(DISTINCT))
    assert same(masked[0].cpu().numpy(), want[0]) and same(masked[1].cpu().numpy(), want[1][:, :3])

    def boom(*a):
        raise AssertionError("the defaults must not reach dllm_token_sample_ex")

    with monkeypatch.context() as mp:
        mp.setattr(L, "dllm_token_sample_ex", boom)
        mp.setattr(L, "dllm_token_sample_ex_workspace", boom)
        tok, st = dllm.sample_tokens(lg, T, 50, SEED, OFFSET)
        assert st.is_contiguous() and tuple(st.shape) == (DISTINCT, 3) and st.dtype == torch.float32
        assert torch.equal(tok, before[0]) and torch.equal(st.view(torch.int32), before[1].view(torch.int32))
        tok, st = dllm.sample_tokens(lg, T, 50, SEED, OFFSET, top_p=1.0, min_p=0.0)
        assert torch.equal(tok, before[0]) and torch.equal(st.view(torch.int32), before[1].view(torch.int32))
        with pytest.raises(AssertionError):
            dllm.sample_tokens(lg, T, 50, SEED, OFFSET, min_p=0.1)


def test_graph_replay_gives_the_same_bits(dllm, cuda):
    """Captured on its first call on the capture stream (no warm-up of that stream's workspace): no
    allocation through the C ABI, no synchronisation; the replay writes the eager call's bits, and no
    device memory is allocated between the replays."""
    import torch
    V = 50257
    lg = torch.from_numpy(base(V).copy()).cuda().half()
    kw = dict(top_p=0.95, min_p=0.05, return_tau=True)
    eager = dllm.sample_tokens(lg, T, 50, SEED, OFFSET, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):             # a capture stream of its own, whose workspace is new
        gt, gs = dllm.sample_tokens(lg, T, 50, SEED, OFFSET, **kw)
    allocated = torch.cuda.memory_allocated()
    for _ in range(2):
        gt.zero_(), gs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == allocated
        for got, e in zip((gt, gs), eager):
            assert torch.equal(got.view(torch.int32), e.view(torch.int32))
    want = expect(V, 50, 0.95, 0.05, np.arange(DISTINCT))
    assert same(gt.cpu().numpy(), want[0]) and same(gs.cpu().numpy(), want[1])
