"""GPU suite of the row-against-row cosine (include/dllm_quant.h 8l, csrc/neighbors.hip): every test
compares idx and score BITS with tests/neighbors_ref.py.

The kernel's tiles, which the sizes below are chosen around:
  * one v_mfma_i32_16x16x64_i8 covers 16 query rows x 16 store rows x 64 bytes of k; a lane's fragment is
    16 contiguous bytes of one row (so dims around 16, 64 and 128 are the edges of a fragment and of a step);
  * a wave owns 32 x 32 (2 x 2 MFMA tiles), a workgroup of 4 waves 64 query rows x 64 store rows: rows and
    blocks of 31 / 32 / 33 and 63 / 64 / 65 are the one-past-the-edge cases beyond the 15 / 16 / 17 of one
    MFMA tile, and ROWS / BLOCKS below hold them;
  * three load paths: 16-byte (dim % 16 == 0, codes 16-byte aligned), dword (dim % 4 == 0, 4-byte aligned)
    and bytes (everything else);
  * the select passes are search's: slices of 2048 keys (rows 2047 / 2049 / 4101: one, two and three
    slices, i.e. one and two passes)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import neighbors_ref as ref

pytestmark = pytest.mark.gpu
NINF = -math.inf


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(rows, dim, seed=0, bits_=8):
    codes, scales, zps = ref.store(rows, dim, seed=7919 * seed + 31 * rows + dim, bits=bits_)
    out = codes, scales, zps, ref.table(codes, scales, zps)
    for a in (codes, scales, zps) + tuple(out[3]):
        a.setflags(write=False)
    return out


def dev(*arrays):
    import torch
    return [torch.tensor(np.ascontiguousarray(a)).cuda() for a in arrays]


def entries(t):
    """A device pair table as ENTRY records."""
    return np.frombuffer(t.cpu().numpy().tobytes(), ref.ENTRY)


def same_table(got, want):
    a, b, c1 = want
    return (np.array_equal(got["a"].view(np.uint64), np.ascontiguousarray(a).view(np.uint64)) and
            np.array_equal(got["b"].view(np.uint64), np.ascontiguousarray(b).view(np.uint64)) and
            np.array_equal(got["c1"].astype(np.int64), c1))


def check(got, sc, k, threshold=NINF, self_base=-1, what=None):
    idx, out = (t.cpu().numpy() for t in got)
    want_idx, want = ref.rank(sc, k, threshold, self_base)
    assert np.array_equal(idx, want_idx), what
    assert np.array_equal(bits(out), bits(want)), what


# ---- every dim ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 15, 16, 17, 63, 64, 65, 127, 128, 260, 263, 768, 775])
def test_bit_exact_every_dim(dllm, cuda, dim):
    rows = 37
    codes, scales, zps, tab = case(rows, dim)
    dc, ds, dz = dev(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    assert same_table(entries(dtab), tab)
    sc = ref.scores(codes, tab, codes, tab)
    for k in (5, rows):
        check(dllm.neighbor_rows(dc, ds, dz, dc, ds, dz, k), sc, k, what=k)
        check(dllm.neighbor_rows(dc, None, None, dc, None, None, k, self_base=0, qtable=dtab, table=dtab), sc, k,
              self_base=0, what=k)


# ---- every row and block count --------------------------------------------------------------------------

ROWS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 257, 2047, 2049, 4101]
BLOCKS = [1, 5, 16, 17, 32, 33, 64, 65, 130]


@pytest.mark.parametrize("rows", ROWS)
def test_bit_exact_every_row_and_block_count(dllm, cuda, rows):
    dim = 64
    codes, scales, zps, tab = case(rows, dim)
    dc, ds, dz = dev(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    assert same_table(entries(dtab), tab)
    ks = sorted({1, min(max(1, rows - 1), 256), min(rows + 3, 256), 256})      # k <= 256
    seen = set()
    for block in BLOCKS:
        nq = min(block, rows)
        for q0 in (0, (rows - nq) // 2, rows - nq):
            if (q0, nq) in seen:
                continue
            seen.add((q0, nq))
            qtab = tuple(t[q0:q0 + nq] for t in tab)
            sc = ref.scores(codes[q0:q0 + nq], qtab, codes, tab)
            for sb in (q0, -1):
                for k in ks:
                    got = dllm.neighbor_rows(dc[q0:q0 + nq], None, None, dc, None, None, k, self_base=sb,
                                             qtable=dtab[q0:q0 + nq], table=dtab)
                    check(got, sc, k, self_base=sb, what=(q0, nq, sb, k))


# ---- operand map ----------------------------------------------------------------------------------------

def test_operand_map(dllm, cuda):
    """Integer-valued rows (s = 1, z = 0).  Query j is one code at position j of the row and nothing
    else, so D[j][t] = q_j c_t[j]: it names the query, the store row and the k position that met.  The
    store's codes differ in every (t, d) and the store is not the queries, so a swapped row / column, a
    k permuted inside the 64-byte step on one operand only, or a wrong lane quarter changes a score."""
    dim, rows = 192, 40
    nq = dim
    q = np.zeros((nq, dim), np.uint8)
    q[np.arange(nq), np.arange(nq)] = 1 + np.arange(nq) % 5
    t, d = np.meshgrid(np.arange(rows), np.arange(dim), indexing="ij")
    c = (1 + (t * 53 + d * 29 + (t * d) % 7) % 250).astype(np.uint8)
    one_q, zero_q = np.ones(nq, np.float32), np.zeros(nq, np.float32)
    one, zero = np.ones(rows, np.float32), np.zeros(rows, np.float32)
    D = ref.dots(q, c)
    assert np.array_equal(D, q[np.arange(nq), np.arange(nq)][:, None].astype(np.float64) * c.T)
    qtab, tab = ref.table(q, one_q, zero_q), ref.table(c, one, zero)
    sc = ref.scores(q, qtab, c, tab)
    assert len(np.unique(sc)) > nq * rows // 4               # the scores do tell the pairs apart
    dq, dc = dev(q, c)
    got = dllm.neighbor_rows(dq, *dev(one_q, zero_q), dc, *dev(one, zero), rows)
    check(got, sc, rows)
    # and the other way round: the store rows as queries (the transposed product)
    got = dllm.neighbor_rows(dc, *dev(one, zero), dq, *dev(one_q, zero_q), nq)
    check(got, ref.scores(c, tab, q, qtab), nq)


# ---- integer range --------------------------------------------------------------------------------------

def test_integer_range_at_the_largest_dim(dllm, cuda):
    """dim 65535: D reaches 65535 * 255^2 > 2^31 and S' = sum (c - 128)(c' - 128) both ends of its range
    (all 0 against all 0: 65535 * 2^14; all 0 against all 255: -65535 * 128 * 127)."""
    dim, rows = 65535, 17
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 256, (rows, dim)).astype(np.uint8)
    codes[0], codes[1], codes[2] = 255, 0, 128
    codes[3, 0::2], codes[3, 1::2] = 0, 255
    codes[4, 0::2], codes[4, 1::2] = 255, 0
    codes[5] = 255
    scales = (0.01 + rng.random(rows)).astype(np.float32)
    zps = rng.standard_normal(rows).astype(np.float32)
    zps[1] = 0.5                                       # the all-zero codes still have a direction
    D = ref.dots(codes, codes)
    assert D.max() == 65535 * 255 ** 2 > 2 ** 31
    tab = ref.table(codes, scales, zps)
    sc = ref.scores(codes, tab, codes, tab)
    dc, ds, dz = dev(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    assert same_table(entries(dtab), tab)
    check(dllm.neighbor_rows(dc, None, None, dc, None, None, rows, qtable=dtab, table=dtab), sc, rows)
    check(dllm.neighbor_rows(dc, None, None, dc, None, None, 4, self_base=0, qtable=dtab, table=dtab), sc, 4, self_base=0)


# ---- ties, threshold, degenerate rows -------------------------------------------------------------------

def test_duplicate_rows_tie_to_the_lower_index(dllm, cuda):
    codes, scales, zps, _ = case(35, 65)
    codes, scales, zps = np.repeat(codes, 2, axis=0), np.repeat(scales, 2), np.repeat(zps, 2)
    tab = ref.table(codes, scales, zps)
    sc = ref.scores(codes, tab, codes, tab)
    dc, ds, dz = dev(codes, scales, zps)
    idx, out = dllm.neighbor_rows(dc, ds, dz, dc, ds, dz, 70)
    check((idx, out), sc, 70)
    idx = idx.cpu().numpy()
    j = np.arange(70)
    assert np.array_equal(idx[:, 0], j & ~1) and np.array_equal(idx[:, 1], j | 1)      # the pair, by index
    idx, out = dllm.neighbor_rows(dc, ds, dz, dc, ds, dz, 70, self_base=0)
    check((idx, out), sc, 70, self_base=0)
    assert np.array_equal(idx.cpu().numpy()[:, 0], j ^ 1)          # the self pair is dropped, its duplicate kept
    assert (idx.cpu().numpy()[:, 69] == -1).all()


def test_threshold(dllm, cuda):
    rows, dim = 70, 64
    codes, scales, zps, tab = case(rows, dim)
    sc = ref.scores(codes, tab, codes, tab)
    dc, ds, dz = dev(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    thr = float(np.sort(sc[3])[-5])                     # one of the reference's own scores
    up = float(np.nextafter(np.float32(thr), np.float32(2)))
    t = int(np.flatnonzero(sc[3] == np.float32(thr))[0])
    for th in (thr, up, NINF, math.inf, 0.0):
        for sb in (-1, 0):
            got = dllm.neighbor_rows(dc, None, None, dc, None, None, rows, threshold=th, self_base=sb, qtable=dtab, table=dtab)
            check(got, sc, rows, th, sb, what=(th, sb))
            idx = got[0].cpu().numpy()
            if th == thr:
                assert t in idx[3]                      # a score equal to the threshold is kept
            if th == up:
                assert t not in idx[3]
            if th == math.inf:
                assert (idx == -1).all() and np.isneginf(got[1].cpu().numpy()).all()
            if th == NINF and sb == -1:
                assert (idx >= 0).all()


def test_degenerate_rows(dllm, cuda):
    """All-zero codes with z = 0 score +0; a constant vector as compress_vectors emits it (s = 0) is its
    zero point; a row with a non-finite s or z scores +0 and disturbs no other row."""
    import torch
    rows, dim = 40, 65
    x = torch.randn(rows, dim, generator=torch.Generator().manual_seed(5)).cuda()
    x[2] = 1.75                                          # constant
    x[7] = 0.0                                           # zero: s = 0, z = 0
    dc, ds, dz = dllm.compress_vectors(x, 8)
    assert float(ds[2]) == 0 and float(dz[2]) == 1.75 and float(ds[7]) == 0 and float(dz[7]) == 0
    ds, dz = ds.clone(), dz.clone()
    ds[11], dz[12], ds[13] = float("nan"), float("inf"), float("-inf")
    codes, scales, zps = dc.cpu().numpy(), ds.cpu().numpy(), dz.cpu().numpy()
    tab = ref.table(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    assert same_table(entries(dtab), tab)
    sc = ref.scores(codes, tab, codes, tab)
    for r in (7, 11, 12, 13):
        assert (bits(sc[r]) == 0).all() and (bits(sc[:, r]) == 0).all()
    assert sc[2, 2] == 1.0
    for sb in (-1, 0):
        check(dllm.neighbor_rows(dc, ds, dz, dc, ds, dz, rows, self_base=sb), sc, rows, self_base=sb)
    keep = [r for r in range(rows) if r not in (7, 11, 12, 13)]
    kt = torch.tensor(keep).cuda()
    check(dllm.neighbor_rows(dc[kt], ds[kt], dz[kt], dc[kt], ds[kt], dz[kt], len(keep)), sc[np.ix_(keep, keep)], len(keep))


# ---- invariances ----------------------------------------------------------------------------------------

def test_slice_invariance(dllm, cuda):
    """A block of queries gives the bits of the whole call; a slice of the store the same scores with
    shifted indices."""
    rows, dim = 2049 + 70, 64
    codes, scales, zps, tab = case(rows, dim)
    dc, ds, dz = dev(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    q = slice(100, 175)
    sc = ref.scores(codes[q], tuple(t[q] for t in tab), codes, tab)
    whole = dllm.neighbor_rows(dc[q], None, None, dc, None, None, 20, self_base=100, qtable=dtab[q], table=dtab)
    check(whole, sc, 20, self_base=100)
    part = dllm.neighbor_rows(dc[130:141], None, None, dc, None, None, 20, self_base=130, qtable=dtab[130:141], table=dtab)
    import torch
    assert torch.equal(part[0], whole[0][30:41]) and torch.equal(part[1].view(torch.int32), whole[1][30:41].view(torch.int32))
    for a, b in [(5, 42), (1000, rows)]:
        n = b - a
        got = dllm.neighbor_rows(dc[q], None, None, dc[a:b], ds[a:b], dz[a:b], min(n, 256), qtable=dtab[q])
        check(got, sc[:, a:b], min(n, 256), what=(a, b))


def test_symmetry(dllm, cuda):
    rows, dim = 67, 263
    codes, scales, zps, tab = case(rows, dim)
    dc, ds, dz = dev(codes, scales, zps)
    idx, out = (t.cpu().numpy() for t in dllm.neighbor_rows(dc, ds, dz, dc, ds, dz, rows - 1, self_base=0))
    full = np.zeros((rows, rows), np.uint32)
    for r in range(rows):
        assert sorted(idx[r].tolist()) == [t for t in range(rows) if t != r]
        full[r, idx[r]] = bits(out[r])
    assert np.array_equal(full, full.T)
    check(dev(idx, out), ref.scores(codes, tab, codes, tab), rows - 1, self_base=0)


@pytest.mark.parametrize("dim", [263, 65, 130])
def test_unaligned_codes(dllm, cuda, dim):
    """The codes of the store and of the queries start one byte past an aligned address and dim % 4 != 0:
    the byte path, the same bits; nothing outside the rows is touched."""
    import torch
    rows, nq = 37, 21
    codes, scales, zps, tab = case(rows, dim)
    qc, qs, qz, qtab = case(nq, dim, seed=1)
    flat = torch.full((rows * dim + 1,), 255, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.tensor(codes).cuda().reshape(-1)
    qflat = torch.full((nq * dim + 1,), 255, dtype=torch.uint8, device="cuda")
    qflat[1:] = torch.tensor(qc).cuda().reshape(-1)
    dc, dq = flat[1:].view(rows, dim), qflat[1:].view(nq, dim)
    assert dc.data_ptr() % 4 == 1 and dq.data_ptr() % 4 == 1 and dc.is_contiguous()
    ds, dz, dqs, dqz = dev(scales, zps, qs, qz)
    dtab = dllm.neighbor_table(dc, ds, dz)
    assert same_table(entries(dtab), tab)
    check(dllm.neighbor_rows(dq, dqs, dqz, dc, None, None, rows, table=dtab), ref.scores(qc, qtab, codes, tab), rows)


# ---- graph capture, the raw entry point -----------------------------------------------------------------

def _raw(dllm, qc, qt, c, t, k, thr, sb, idx, out, ws, wsb, rows=None):
    import torch
    rows = c.shape[0] if rows is None else rows
    return dllm._lib.load().dllm_neighbor_rows(
        C.c_void_p(qc.data_ptr()), C.c_void_p(qt.data_ptr()), qc.shape[0], C.c_void_p(c.data_ptr()),
        C.c_void_p(t.data_ptr()), rows, c.shape[1], k, thr, sb, C.c_void_p(idx.data_ptr()), C.c_void_p(out.data_ptr()),
        C.c_void_p(ws.data_ptr()), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_graph_replay_gives_the_eager_bits(dllm, cuda):
    """Captured after one warm call; three replays, each into cleared outputs."""
    import torch
    rows, dim, k, nq = 2 * 2048 + 5, 64, 10, 70
    codes, scales, zps, tab = case(rows, dim)
    dc, ds, dz = dev(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    eager = dllm.neighbor_rows(dc[:nq], None, None, dc, None, None, k, threshold=0.0, self_base=0, qtable=dtab[:nq], table=dtab)
    wsb = dllm._lib.load().dllm_neighbor_workspace(nq, rows, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    out = torch.full((nq, k), float("nan"), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert _raw(dllm, dc[:nq], dtab[:nq], dc, dtab, k, 0.0, 0, idx, out, ws, wsb) == 0
        for _ in range(3):
            idx.fill_(-7)
            out.fill_(float("nan"))
            ws.zero_()
            graph.replay()
            s.synchronize()
            assert torch.equal(idx, eager[0])
            assert torch.equal(out.view(torch.int32), eager[1].view(torch.int32))
    sc = ref.scores(codes[:nq], tuple(t[:nq] for t in tab), codes, tab)
    check((idx, out), sc, k, 0.0, 0)


def test_empty_store_and_short_workspace(dllm, cuda):
    import torch
    rows, dim, k, nq = 33, 64, 4, 5
    codes, scales, zps, _ = case(rows, dim)
    dc, ds, dz = dev(codes, scales, zps)
    dtab = dllm.neighbor_table(dc, ds, dz)
    idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    out = torch.full((nq, k), 7.0, device="cuda")
    wsb = dllm._lib.load().dllm_neighbor_workspace(nq, rows, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    assert _raw(dllm, dc[:nq], dtab[:nq], dc, dtab, k, NINF, -1, idx, out, ws, wsb - 1) == dllm._lib.ERR_INVALID_PARAMS
    torch.cuda.synchronize()
    assert (idx == -7).all() and (out == 7.0).all()                  # nothing was launched
    assert _raw(dllm, dc[:nq], dtab[:nq], dc, dtab, k, NINF, -1, idx, out, ws, wsb, rows=0) == 0
    torch.cuda.synchronize()
    assert (idx == -1).all() and torch.isneginf(out).all()
    e_idx, e_out = dllm.neighbor_rows(dc[:nq], ds[:nq], dz[:nq], dc[:0], ds[:0], dz[:0], 2)
    assert (e_idx == -1).all() and torch.isneginf(e_out).all()


def test_search_keeps_nan_scores_as_rows(dllm, cuda):
    """The select passes are shared with dllm_search_vectors, where a NaN score is still a row that ranks
    last (8g), not "no row": the flag that drops NaNs is the neighbour path's alone."""
    import torch
    from tests import search_ref
    codes, scales, zps = search_ref.store(9, 64, seed=4)
    Q = np.random.default_rng(4).standard_normal((2, 64)).astype(np.float32)
    Q[1, 5] = np.nan
    idx, out = dllm.search_vectors(*dev(Q, codes, scales, zps), 9)
    assert idx[1].cpu().tolist() == list(range(9)) and torch.isnan(out[1]).all()
    assert (idx[0] >= 0).all() and torch.isfinite(out[0]).all()


# ---- VectorIndex ----------------------------------------------------------------------------------------

def test_build_graph_end_to_end(dllm, cuda):
    """300 rows x dim 48 at block 128 (three blocks, the last ragged), non-contiguous ids; again after an
    insert_batch that replaces a row, so the cached pair table is rebuilt."""
    import torch
    n, dim, k = 300, 48, 12        # clusters of 10: nine mates above the threshold, so the last places stay empty
    g = torch.Generator().manual_seed(11)
    base = torch.randn(30, dim, generator=g)
    x = (base[torch.arange(n) % 30] + 0.25 * torch.randn(n, dim, generator=g)).cuda()      # clusters: edges above 0.8 exist
    ids = [5000 + 7 * i for i in range(n)]
    ix = dllm.VectorIndex(dim, 8)
    ix.insert_batch(ids[:170], x[:170])
    ix.insert_batch(ids[170:], x[170:])

    def expect():
        codes, scales, zps = (t[:n].cpu().numpy() for t in (ix._codes, ix._scales, ix._zps))
        tab = ref.table(codes, scales, zps)
        return ref.rank(ref.scores(codes, tab, codes, tab), k, 0.8, 0)

    for round_ in range(2):
        graph = ix.build_graph(k, threshold=0.8, block=128)
        want_idx, want = expect()
        assert graph.ids == ids and len(graph) == n
        assert np.array_equal(graph.idx.cpu().numpy(), want_idx) and np.array_equal(bits(graph.scores.cpu().numpy()), bits(want))
        assert (want_idx[:, 0] >= 0).sum() > n // 2            # the threshold leaves real edges ...
        assert (want_idx[:, k - 1] == -1).any()                # ... and drops some
        r = int(np.flatnonzero(want_idx[:, 1] >= 0)[0])
        assert [i for i, _ in graph.neighbors(ids[r])] == [ids[t] for t in want_idx[r] if t >= 0]
        assert graph.neighbors(1) == []
        e = graph.edges()
        assert len(e) == int((want_idx >= 0).sum()) and all(a != b and w >= 0.8 for a, b, w in e)
        whole = ix.build_graph(k)                              # the default block and threshold: one call
        assert torch.equal(whole.idx, graph.idx) and torch.equal(whole.scores.view(torch.int32), graph.scores.view(torch.int32))
        got = ix.neighbors([ids[r], 3, ids[299]], k, threshold=0.8)
        assert got[1] == [] and [i for i, _ in got[0]] == [ids[t] for t in want_idx[r] if t >= 0]
        assert [i for i, _ in got[2]] == [ids[t] for t in want_idx[299] if t >= 0]
        if round_ == 0:                                        # id 5007 (row 1) takes row 200's vector: a new nearest pair
            before = graph.neighbors(ids[200])
            ix.insert_batch([ids[1]], x[200:201])
            assert len(ix) == n
    assert graph.neighbors(ids[200])[0][0] == ids[1] and graph.neighbors(ids[200]) != before
