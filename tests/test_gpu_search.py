"""GPU suite of the compressed-vector search: dllm_search_table / dllm_search_vectors bit for bit
against the numpy restatement of the score rule (tests/search_ref.py) at the smallest sizes that
reach each part of the kernels, order-sensitive queries, slice invariance, table reuse, graph
capture, the empty store, and VectorIndex end to end.

Sizes the kernels turn on: a strand trip is 256 codes; a scan wave holds 8 rows and a scan
workgroup 32; a pass holds 4 queries (then 2, then 1); a select slice is S = 2048 keys, and more
than S surviving candidates take another select pass."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import search_ref as ref

pytestmark = pytest.mark.gpu

S = 2048
# one element; one group; a quarter trip; the trip edge from both sides (252, 256) and a strand's
# second trip (260); the default hidden size; 263 and 775 are no multiples of 4, so rows start at odd
# byte offsets and the last group is ragged.
DIMS = [1, 4, 64, 252, 256, 260, 263, 768, 775]
# 9 = one more than a wave's rows, 33 = one more than a workgroup's; 2 S + 5 takes three slices.
ROWS = [1, 3, 9, 33, S - 1, S, S + 1, 2 * S + 5]
NQ = 5          # one more than the query tile: a pass of 4 and a pass of 1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(rows, dim):
    """(Q, codes, scales, zps, scores [NQ, rows]): computed once, never written to."""
    codes, scales, zps = ref.store(rows, dim, seed=rows * 1000 + dim)
    Q = np.random.default_rng(dim * 7 + rows).standard_normal((NQ, dim)).astype(np.float32)
    out = Q, codes, scales, zps, ref.scores(Q, codes, ref.table(codes, scales, zps))
    for a in out:
        a.setflags(write=False)
    return out


def dev(*arrays):
    import torch
    return [torch.tensor(a).cuda() for a in arrays]


def check(got, sc, k):
    idx, out = (t.cpu().numpy() for t in got)
    want_idx, want = ref.topk(sc, k)
    assert idx.dtype == np.int32 and out.dtype == np.float32 and idx.shape == want_idx.shape
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(bits(out), bits(want))


@pytest.mark.parametrize("dim", DIMS)
def test_bit_exact_every_dim(dllm, cuda, dim):
    rows = 37
    Q, codes, scales, zps, sc = case(rows, dim)
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    tab = dllm.search_table(dc, ds, dz)
    assert np.array_equal(bits(tab.cpu().numpy()), bits(ref.table(codes, scales, zps)))
    check(dllm.search_vectors(dQ, dc, ds, dz, 5), sc, 5)
    check(dllm.search_vectors(dQ, dc, ds, dz, rows), sc, rows)     # the whole score matrix, ranked


@pytest.mark.parametrize("rows", ROWS)
def test_bit_exact_every_row_count(dllm, cuda, rows):
    dim = 64
    Q, codes, scales, zps, sc = case(rows, dim)
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    ks = sorted({1, min(rows, 256), 256, min(rows + 3, 256)})       # 1, rows, 256, and k > rows
    for nq in (1, 2, NQ):
        for k in ks:
            check(dllm.search_vectors(dQ[:nq], dc, ds, dz, k), sc[:nq], k)
    idx, out = dllm.search_vectors(dQ[1], dc, ds, dz, 3)             # a 1-D query returns 1-D results
    assert idx.shape == (3,) and out.shape == (3,)
    check((idx[None], out[None]), sc[1:2], 3)


def test_second_select_pass(dllm, cuda):
    """8 S + 1 rows at k = 256: nine slices leave 2304 > S candidates, so the select runs three
    times (9 slices, 2 slices, 1)."""
    rows, dim = 8 * S + 1, 4
    Q, codes, scales, zps, sc = case(rows, dim)
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    check(dllm.search_vectors(dQ[:2], dc, ds, dz, 256), sc[:2], 256)


def test_unaligned_codes_and_queries(dllm, cuda):
    """dim % 4 == 0 but the codes start one byte, the queries one float, past an aligned address:
    the byte path, the same bits."""
    import torch
    rows, dim = 37, 260
    Q, codes, scales, zps, sc = case(rows, dim)
    flat = torch.zeros(rows * dim + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.tensor(codes).cuda().reshape(-1)
    dc = flat[1:].view(rows, dim)
    qflat = torch.zeros(NQ * dim + 1, device="cuda")
    qflat[1:] = torch.tensor(Q).cuda().reshape(-1)
    dQ = qflat[1:].view(NQ, dim)
    assert dc.data_ptr() % 4 == 1 and dQ.data_ptr() % 16 == 4 and dc.is_contiguous()
    ds, dz = dev(scales, zps)
    tab = dllm.search_table(dc, ds, dz)
    assert np.array_equal(bits(tab.cpu().numpy()), bits(ref.table(codes, scales, zps)))
    check(dllm.search_vectors(dQ, dc, ds, dz, 7, table=tab), sc, 7)


@pytest.mark.parametrize("dim", [768, 775])
def test_order_patterns(dllm, cuda, dim):
    """Queries whose strand sums move with the order of the sum (the CPU suite shows which
    reorderings they catch): a wrong lane mapping, chain or tree fails rather than passes by luck."""
    rows = 9
    _, codes, scales, zps, _ = case(rows, dim)
    dc, ds, dz = dev(codes, scales, zps)
    tab = ref.table(codes, scales, zps)
    dtab = dllm.search_table(dc, ds, dz)
    for mask in ref.MASKS:
        for seed in range(2):
            Q = ref.order_pattern(NQ, dim, seed, mask)
            got = dllm.search_vectors(torch_of(Q), dc, ds, dz, rows, table=dtab)
            check(got, ref.scores(Q, codes, tab), rows)


def torch_of(a):
    import torch
    return torch.tensor(a).cuda()


def test_slice_invariance(dllm, cuda):
    """A score depends on its query and row alone: rows [a, b) searched on their own, at another
    place in another grid, give the bits they have inside the whole store."""
    rows, dim = S + 1, 64
    Q, codes, scales, zps, sc = case(rows, dim)
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    for a, b in [(5, 42), (1000, S + 1)]:
        n = b - a
        check(dllm.search_vectors(dQ[:3], dc[a:b], ds[a:b], dz[a:b], min(n, 256)), sc[:3, a:b], min(n, 256))


def test_table_reuse(dllm, cuda):
    import torch
    rows, dim = 33, 256
    Q, codes, scales, zps, sc = case(rows, dim)
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    tab = dllm.search_table(dc, ds, dz)
    a = dllm.search_vectors(dQ, dc, ds, dz, 10)
    b = dllm.search_vectors(dQ, dc, ds, dz, 10, table=tab)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    check(b, sc, 10)


def test_non_finite_and_zero_queries(dllm, cuda):
    """On the device as on the host: a NaN in a query makes its scores NaN, ranked by index; a zero
    query scores +0 everywhere; the other queries of the batch are untouched."""
    rows, dim = 33, 260
    Q, codes, scales, zps, sc = case(rows, dim)
    Q = Q.copy()
    Q[1, 259] = np.nan
    Q[2] = 0
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    idx, out = (t.cpu().numpy() for t in dllm.search_vectors(dQ, dc, ds, dz, 6))
    assert np.isnan(out[1]).all() and idx[1].tolist() == list(range(6))
    assert (bits(out[2]) == 0).all() and idx[2].tolist() == list(range(6))
    check((torch_of(idx[[0, 3, 4]]), torch_of(out[[0, 3, 4]])), sc[[0, 3, 4]], 6)


def _raw(dllm, Q, codes, tab, k, idx, out, ws, wsb, rows=None):
    import torch
    rows = codes.shape[0] if rows is None else rows
    return dllm._lib.load().dllm_search_vectors(
        C.c_void_p(Q.data_ptr()), Q.shape[0], C.c_void_p(codes.data_ptr()), C.c_void_p(tab.data_ptr()), rows,
        Q.shape[1], k, C.c_void_p(idx.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), wsb,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_graph_replay_gives_the_eager_bits(dllm, cuda):
    """Captured after one warm call; three replays, each into cleared outputs."""
    import torch
    rows, dim, k = 2 * S + 5, 64, 10
    Q, codes, scales, zps, sc = case(rows, dim)
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    tab = dllm.search_table(dc, ds, dz)
    eager = dllm.search_vectors(dQ, dc, ds, dz, k, table=tab)
    wsb = dllm._lib.load().dllm_search_workspace(NQ, rows, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    idx = torch.full((NQ, k), -7, dtype=torch.int32, device="cuda")
    out = torch.full((NQ, k), float("nan"), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert _raw(dllm, dQ, dc, tab, k, idx, out, ws, wsb) == 0
        for _ in range(3):
            idx.fill_(-7)
            out.fill_(float("nan"))
            ws.zero_()
            graph.replay()
            s.synchronize()
            assert torch.equal(idx, eager[0])
            assert torch.equal(out.view(torch.int32), eager[1].view(torch.int32))
    check((idx, out), sc, k)


def test_empty_store_and_short_workspace(dllm, cuda):
    import torch
    rows, dim, k = 33, 64, 4
    Q, codes, scales, zps, _ = case(rows, dim)
    dQ, dc, ds, dz = dev(Q, codes, scales, zps)
    tab = dllm.search_table(dc, ds, dz)
    idx = torch.full((NQ, k), -7, dtype=torch.int32, device="cuda")
    out = torch.full((NQ, k), 7.0, device="cuda")
    wsb = dllm._lib.load().dllm_search_workspace(NQ, rows, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    assert _raw(dllm, dQ, dc, tab, k, idx, out, ws, wsb - 1) == dllm._lib.ERR_INVALID_PARAMS
    torch.cuda.synchronize()
    assert (idx == -7).all() and (out == 7.0).all()                  # nothing was launched
    assert _raw(dllm, dQ, dc, tab, k, idx, out, ws, wsb, rows=0) == 0
    torch.cuda.synchronize()
    assert (idx == -1).all() and torch.isneginf(out).all()
    e_idx, e_out = dllm.search_vectors(dQ, dc[:0], ds[:0], dz[:0], 2)
    assert (e_idx == -1).all() and torch.isneginf(e_out).all()


def test_vector_index_end_to_end(dllm, cuda):
    """insert, replace, get and search on the device; the ids agree with torch.topk over the cosine
    of the decompressed rows on well-separated random rows."""
    import torch
    dim, n, k = 96, 300, 5
    g = torch.Generator().manual_seed(27)
    x = torch.randn(n, dim, generator=g).cuda()
    ids = [1000 + 3 * i for i in range(n)]
    ix = dllm.VectorIndex(dim, 8)
    ix.insert_batch(ids[:200], x[:200])
    ix.insert_batch(ids[200:], x[200:])
    assert len(ix) == n and ix.size_bytes() == n * dim + sum(len(str(i)) for i in ids)
    # a stored vector comes back as compress + decompress leaves it; a missing id as zeros
    got = ix.get_batch([ids[7], 5, ids[250]])
    c, s, z = dllm.compress_vectors(x[[7, 250]], 8)
    assert torch.equal(got[[0, 2]], dllm.decompress_vectors(c, s, z)) and (got[1] == 0).all()
    # a query near a stored vector finds it first, with a cosine near 1
    q = x[123] + 0.05 * torch.randn(dim, generator=g).cuda()
    hits = ix.search(q, k)
    assert len(hits) == k and hits[0][0] == ids[123] and 0.99 < hits[0][1] <= 1.0 + 1e-5
    assert all(a[1] >= b[1] for a, b in zip(hits, hits[1:]))
    # replacing id 123's vector moves it: the old neighbour is gone, the new one is found
    ix.insert_batch([ids[123]], -x[123:124])
    assert len(ix) == n
    assert ix.search(q, k)[0][0] != ids[123]
    assert ix.search(-q, 1)[0][0] == ids[123]
    # against torch over the decompressed store (random 96-d rows: cosine gaps ~1e-2 >> the 1e-5 bound)
    Q = torch.randn(4, dim, generator=g).cuda()
    rows = ix.get_batch(ids).double()
    cos = torch.nn.functional.normalize(Q.double(), dim=1) @ torch.nn.functional.normalize(rows, dim=1).T
    top = torch.topk(cos, k + 1, dim=1)
    gap = float((top.values[:, :-1] - top.values[:, 1:]).min())
    print("smallest gap among the top", k + 1, "cosines:", gap)
    assert gap > 2e-4          # the data is what the comparison needs: no near-ties (the rule's bound is ~1e-5)
    res = ix.search_batch(Q, k)
    for j in range(4):
        assert [h[0] for h in res[j]] == [ids[i] for i in top.indices[j, :k].tolist()]
        assert np.allclose([h[1] for h in res[j]], top.values[j, :k].cpu().numpy(), atol=2e-5, rtol=0)
    # k beyond the store: every stored id once, nothing more
    small = dllm.VectorIndex(dim, 4)
    small.insert_batch([1, 2, 3], x[:3])
    assert sorted(h[0] for h in small.search(x[0], 10)) == [1, 2, 3]
    assert dllm.VectorIndex(dim, 4).search(x[0], 3) == []
