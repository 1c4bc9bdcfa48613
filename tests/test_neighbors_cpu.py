"""CPU suite of the row-against-row cosine (include/dllm_quant.h 8l): the two restatements of the rule
(tests/neighbors_ref.py) agree bit for bit, the host entry points dllm_neighbor_table_host /
dllm_neighbor_rows_host match them bit for bit, the bits are symmetric, the rule stays within the
header's derived bound of the exact rational cosine and within the sum of the two headers' bounds of
8g's score, the C entry points reject what the header says they reject, in its order, before any
device work, and the VectorIndex / NavigationGraph bookkeeping.  No GPU work here."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import neighbors_ref as ref
from tests import search_ref
from tests.host_check import run_host_check

DIMS = [1, 3, 16, 63, 64, 65, 263, 768]
NINF = -math.inf


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(dim, rows=9, bits_=8, kind="normal"):
    """(codes, scales, zps, table, scores of the store against itself): computed once, never written to."""
    codes, scales, zps = ref.store(rows, dim, seed=1000 * bits_ + dim, bits=bits_, kind=kind)
    tab = ref.table(codes, scales, zps)
    out = codes, scales, zps, tab, ref.scores(codes, tab, codes, tab)
    for a in (codes, scales, zps, out[4]) + tuple(tab):
        a.setflags(write=False)
    return out


def host_table(L, codes, scales, zps):
    codes, scales, zps = (np.ascontiguousarray(a) for a in (codes, scales, zps))
    rows, dim = codes.shape
    assert L.dllm_neighbor_table_bytes(rows) == rows * ref.ENTRY.itemsize
    tab = np.zeros(rows, ref.ENTRY)
    assert L.dllm_neighbor_table_host(codes.ctypes.data, rows, dim, scales.ctypes.data, zps.ctypes.data,
                                      tab.ctypes.data) == 0, L.dllm_last_error()
    return tab


def host_rows(L, qcodes, qtab, codes, tab, k, threshold=NINF, self_base=-1):
    qcodes, qtab, codes, tab = (np.ascontiguousarray(a) for a in (qcodes, qtab, codes, tab))
    nq, (rows, dim) = qcodes.shape[0], codes.shape
    idx = np.full((nq, k), 77, np.int32)
    sc = np.full((nq, k), 77, np.float32)
    rc = L.dllm_neighbor_rows_host(qcodes.ctypes.data, qtab.ctypes.data, nq, codes.ctypes.data if rows else None,
                                   tab.ctypes.data if rows else None, rows, dim, k, threshold, self_base,
                                   idx.ctypes.data, sc.ctypes.data)
    assert rc == 0, L.dllm_last_error()
    return idx, sc


def same_table(got, want):
    """A host / device table (ENTRY records) against the reference's (a, b, C1): f64 bits and C1."""
    a, b, c1 = want
    return (np.array_equal(got["a"].view(np.uint64), np.ascontiguousarray(a).view(np.uint64)) and
            np.array_equal(got["b"].view(np.uint64), np.ascontiguousarray(b).view(np.uint64)) and
            np.array_equal(got["c1"].astype(np.int64), c1))


# ---- the restatements -------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 64, 65, 263])
def test_restatements_agree(dim):
    codes, scales, zps, tab, sc = case(dim, rows=6)
    loop = ref.table_loop(codes, scales, zps)
    assert same_table(ref.table_bytes(tuple(np.array(c) for c in zip(*loop))), tab)
    assert np.array_equal(bits(sc), bits(ref.scores_loop(codes, loop, codes, loop)))
    thr = float(np.sort(sc[0])[2])
    for k, t, sb in [(1, NINF, -1), (4, NINF, 0), (9, NINF, -1), (9, thr, 0), (3, math.inf, -1)]:
        a, b = ref.rank(sc, k, t, sb), ref.rank_loop(sc, k, t, sb)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (k, t, sb)


def test_restatements_agree_on_degenerate_rows():
    codes = np.zeros((5, 8), np.uint8)
    codes[1:] = np.random.default_rng(0).integers(0, 256, (4, 8))
    scales = np.array([0.5, 0.0, np.nan, 1.0, 3e38], np.float32)
    zps = np.array([0.0, 2.0, 1.0, np.inf, 3e38], np.float32)
    tab, loop = ref.table(codes, scales, zps), ref.table_loop(codes, scales, zps)
    assert same_table(ref.table_bytes(tuple(np.array(c) for c in zip(*loop))), tab)
    assert tab[0][0] == 0 and tab[0][2] == 0 and tab[0][3] == 0   # no direction -> a = b = +0
    sc = ref.scores(codes, tab, codes, tab)
    assert np.array_equal(bits(sc), bits(ref.scores_loop(codes, loop, codes, loop)))
    assert not np.isnan(sc).any()


# ---- the host entry points --------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", [5, 40])
def test_host_matches_restatement(dllm, dim, rows):
    L = dllm._lib.load()
    codes, scales, zps, tab, sc = case(dim, rows=rows)
    got = host_table(L, codes, scales, zps)
    assert same_table(got, tab)
    for k, sb, q0, nq in [(1, -1, 0, rows), (5, 0, 0, rows), (rows + 3, 2, 2, 3), (rows, -1, 1, 2)]:
        idx, out = host_rows(L, codes[q0:q0 + nq], got[q0:q0 + nq], codes, got, k, NINF, sb)
        want_idx, want = ref.rank(sc[q0:q0 + nq], k, NINF, sb)
        assert np.array_equal(idx, want_idx), (k, sb)
        assert np.array_equal(bits(out), bits(want)), (k, sb)


def test_host_threshold_and_ties(dllm):
    L = dllm._lib.load()
    codes, scales, zps, _, _ = case(64, rows=6)
    codes, scales, zps = np.repeat(codes[:3], 2, axis=0), np.repeat(scales[:3], 2), np.repeat(zps[:3], 2)
    tab = host_table(L, codes, scales, zps)
    sc = ref.scores(codes, ref.table(codes, scales, zps), codes, ref.table(codes, scales, zps))
    idx, out = host_rows(L, codes, tab, codes, tab, 6, NINF, 0)
    want_idx, want = ref.rank(sc, 6, NINF, 0)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(out), bits(want))
    for j in range(6):                       # the self pair is dropped, its duplicate kept and first
        assert idx[j, 0] == (j ^ 1) and idx[j, 5] == -1 and np.isneginf(out[j, 5])
    thr = float(sc[0, 2])
    for t in (thr, float(np.nextafter(np.float32(thr), np.float32(2))), math.inf, NINF):
        idx, out = host_rows(L, codes, tab, codes, tab, 6, t, -1)
        want_idx, want = ref.rank(sc, 6, t, -1)
        assert np.array_equal(idx, want_idx) and np.array_equal(bits(out), bits(want)), t
    assert 2 in host_rows(L, codes[:1], tab[:1], codes, tab, 6, thr, -1)[0][0]
    assert 2 not in host_rows(L, codes[:1], tab[:1], codes, tab, 6, float(np.nextafter(np.float32(thr), np.float32(2))), -1)[0][0]


def test_host_degenerate_rows(dllm):
    """Zero codes with z = 0, a constant row (s = 0) and non-finite rows: +0 against everything, and the
    other rows' scores are those of a store without them."""
    L = dllm._lib.load()
    codes, scales, zps, _, _ = case(65, rows=7)
    codes, scales, zps = codes.copy(), scales.copy(), zps.copy()
    codes[1] = 0
    zps[1] = 0
    scales[2] = 0
    codes[2] = 0
    scales[3] = np.nan
    zps[4] = np.inf
    tab = host_table(L, codes, scales, zps)
    rt = ref.table(codes, scales, zps)
    assert same_table(tab, rt)
    sc = ref.scores(codes, rt, codes, rt)
    idx, out = host_rows(L, codes, tab, codes, tab, 7)
    want_idx, want = ref.rank(sc, 7)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(out), bits(want))
    for r in (1, 3, 4):
        assert (bits(sc[r]) == 0).all() and (bits(sc[:, r]) == 0).all()
    assert abs(sc[2, 2] - 1) < 1e-6          # the constant row is its zero point: a direction
    keep = [0, 2, 5, 6]
    sub = ref.scores(codes[keep], ref.table(codes[keep], scales[keep], zps[keep]), codes[keep],
                     ref.table(codes[keep], scales[keep], zps[keep]))
    assert np.array_equal(bits(sub), bits(sc[np.ix_(keep, keep)]))


@pytest.mark.parametrize("dim", [37, 768])
def test_symmetry_of_the_bits(dim):
    for b in (1, 8):
        sc = case(dim, rows=12, bits_=b)[4]
        assert np.array_equal(bits(sc), bits(sc.T))


# ---- the bounds -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["normal", "offset"])
@pytest.mark.parametrize("b", [1, 2, 4, 8])
def test_rule_within_derived_bound(kind, b):
    """|score - exact rational cosine| <= 2^-25 + 12 u kr kt + 2^-51 (kr^3 + kt^3) / 2 (the header's 8l)."""
    worst = 0.0
    for dim, rows in ((37, 6), (768, 3)):
        codes, scales, zps, tab, sc = case(dim, rows=rows, bits_=b, kind=kind)
        kap = ref.kappa(codes, scales, zps)
        lim = ref.bound(kap[:, None], kap[None, :])
        assert lim.max() < 2.0 ** -24, "the derivation would be wrong"
        for r in range(rows):
            for t in range(rows):
                exact = ref.cosine_exact(codes[r], scales[r], zps[r], codes[t], scales[t], zps[t])
                err = abs(float(sc[r, t]) - exact)
                worst = max(worst, err)
                assert err <= lim[r, t], (dim, r, t, err, lim[r, t])
    print(kind, b, "worst err", worst)


@pytest.mark.parametrize("kind", ["normal", "offset"])
def test_cross_check_against_search_rule(kind):
    """score_8l(r, t) against 8g's score of the decompressed row r as the query.  Three gaps add up:
      |score_8l - cos(v_r, v_t)|          <= bound_8l(kr, kt), v the algebraic rows s c + z;
      |score_8g - cos(dec_r, dec_t)|      <= bound_8g(dim, kt), dec the f32 rows of decompress (8g's bound
                                             is against the decompressed store row and already holds the
                                             4 kt 2^-24 of that row's two roundings per element);
      |cos(dec_r, v_t) - cos(v_r, v_t)|   <= |dec_r - v_r| / |v_r| <= 2^-23 kr: an element of dec_r is
                                             RN(RN(c s) + z), off by at most 2^-24 (2 |c s| + |z|), so the
                                             query moves by at most 2^-23 kr |v_r|, and a cosine moves by
                                             at most the relative move of one of its vectors.
    The sum: bound_8l + bound_8g + 2^-23 kr."""
    rows, dim = 24, 768
    codes, scales, zps, tab, sc = case(dim, rows=rows, kind=kind)
    Q = search_ref.decompress(codes, scales, zps)
    sg = search_ref.scores(Q, codes, search_ref.table(codes, scales, zps))
    kap = ref.kappa(codes, scales, zps)
    lim = ref.bound(kap[:, None], kap[None, :]) + search_ref.bound(dim, kap)[None, :] + 2.0 ** -23 * kap[:, None]
    err = np.abs(sc.astype(np.float64) - sg.astype(np.float64))
    print(kind, "max diff", err.max(), "min bound", lim.min())
    assert (err <= lim).all()
    assert lim.max() < 1e-3


# ---- the error contract, through the C entry points, nothing launched -------------------------------

def test_neighbor_rows_rejections_in_order(dllm):
    L = dllm._lib.load()
    INV, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)       # never dereferenced: every call below returns before a launch
    ws = L.dllm_neighbor_workspace(2, 10, 3)

    def call(qc=p, qt=p, nq=2, codes=p, table=p, rows=10, dim=8, k=3, thr=0.5, sb=-1, idx=p, scores=p, w=p, wb=ws):
        return L.dllm_neighbor_rows(qc, qt, nq, codes, table, rows, dim, k, thr, sb, idx, scores, w, wb, None)

    # each check alone
    assert call(k=0) == INV and call(k=257) == INV and b"between 1 and 256" in L.dllm_last_error()
    assert call(dim=0) == INV and call(dim=65536) == INV
    assert call(rows=2 ** 31, wb=2 ** 62) == SHAPE
    assert call(thr=math.nan) == INV and b"NaN" in L.dllm_last_error()
    assert call(sb=-2) == INV
    assert call(sb=9) == INV and b"self_base" in L.dllm_last_error()
    assert call(sb=11) == INV
    assert call(nq=0) == 0
    assert call(nq=0, qc=None, qt=None, idx=None, scores=None, w=None, wb=0) == 0
    for name in ("qc", "qt", "codes", "table", "idx", "scores"):
        assert call(**{name: None}) == INV and b"NULL" in L.dllm_last_error(), name
    assert call(qt=C.c_void_p(4100)) == INV and call(table=C.c_void_p(4100)) == INV
    assert call(w=None) == INV and b"workspace" in L.dllm_last_error()
    assert call(wb=ws - 1) == INV and call(w=C.c_void_p(4104)) == INV
    # the order: k, dim, rows, threshold, self_base, nq == 0, NULL, workspace
    assert call(k=0, dim=0, rows=2 ** 31) == INV and b"k must" in L.dllm_last_error()
    assert call(dim=0, rows=2 ** 31) == INV and b"dim" in L.dllm_last_error()
    assert call(rows=2 ** 31, thr=math.nan) == SHAPE
    assert call(thr=math.nan, sb=-5) == INV and b"NaN" in L.dllm_last_error()
    assert call(sb=-5, nq=0) == INV
    assert call(sb=9, nq=0) == 0 and call(sb=11, nq=0) == INV          # self_base + nq > rows comes before nq == 0
    assert call(qc=None, w=None) == INV and b"NULL" in L.dllm_last_error()
    # the table entry point
    assert L.dllm_neighbor_table(None, 4, 8, p, p, p, None) == INV
    assert L.dllm_neighbor_table(p, 4, 8, p, p, None, None) == INV
    assert L.dllm_neighbor_table(p, 4, 0, p, p, p, None) == INV
    assert L.dllm_neighbor_table(p, 2 ** 31, 8, p, p, p, None) == SHAPE
    assert L.dllm_neighbor_table(p, 4, 8, p, p, C.c_void_p(4100), None) == INV
    assert L.dllm_neighbor_table(None, 0, 8, None, None, None, None) == 0


def test_host_rejections_leave_outputs_untouched(dllm):
    L = dllm._lib.load()
    INV, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_SHAPE_MISMATCH
    codes, scales, zps, _, _ = case(16, rows=5)
    codes = np.ascontiguousarray(codes)
    tab = host_table(L, codes, scales, zps)
    idx = np.full((2, 3), 77, np.int32)
    sc = np.full((2, 3), 77, np.float32)

    def call(qc=codes.ctypes.data, qt=tab.ctypes.data, nq=2, c=codes.ctypes.data, t=tab.ctypes.data, rows=5, dim=16, k=3,
             thr=0.0, sb=-1, i=idx.ctypes.data, s=sc.ctypes.data):
        return L.dllm_neighbor_rows_host(qc, qt, nq, c, t, rows, dim, k, thr, sb, i, s)

    want = [(dict(k=0), INV), (dict(k=257), INV), (dict(dim=0), INV), (dict(dim=65536), INV), (dict(rows=2 ** 31), SHAPE),
            (dict(thr=math.nan), INV), (dict(sb=-2), INV), (dict(sb=4), INV), (dict(qc=None), INV), (dict(qt=None), INV),
            (dict(c=None), INV), (dict(t=None), INV), (dict(qt=tab.ctypes.data + 4), INV), (dict(nq=0), 0),
            (dict(k=0, dim=0, rows=2 ** 31, thr=math.nan, sb=-2), INV), (dict(rows=2 ** 31, thr=math.nan), SHAPE)]
    for kw, rc in want:
        assert call(**kw) == rc, kw
        assert (idx == 77).all() and (sc == 77).all(), kw
    assert call(i=None) == INV and call(s=None) == INV
    assert call(sb=3) == 0 and (idx != 77).all()
    t2 = np.full(5, 7, ref.ENTRY)
    assert L.dllm_neighbor_table_host(None, 5, 16, scales.ctypes.data, zps.ctypes.data, t2.ctypes.data) == INV
    assert L.dllm_neighbor_table_host(codes.ctypes.data, 5, 0, scales.ctypes.data, zps.ctypes.data, t2.ctypes.data) == INV
    assert L.dllm_neighbor_table_host(codes.ctypes.data, 2 ** 31, 16, scales.ctypes.data, zps.ctypes.data, t2.ctypes.data) == SHAPE
    assert (t2["c1"] == 7).all()


def test_workspace_query(dllm):
    """Scores f32 [nq][rows] rounded up to 16 bytes + the candidate keys of search's select passes."""
    L = dllm._lib.load()
    up = lambda b: -(-b // 16) * 16
    assert L.dllm_neighbor_workspace(1, 10, 3) == up(40)
    assert L.dllm_neighbor_workspace(3, 2048, 256) == up(3 * 2048 * 4)
    assert L.dllm_neighbor_workspace(3, 2049, 256) == up(3 * 2049 * 4) + 3 * 2 * 256 * 8
    for nq, rows, k in [(1, 1, 1), (5, 4101, 256), (256, 1 << 16, 10)]:
        assert L.dllm_neighbor_workspace(nq, rows, k) == L.dllm_search_workspace(nq, rows, k) - up(8 * nq)


# ---- the Python surface -----------------------------------------------------------------------------

def test_wrappers_exported(dllm):
    for name in ("neighbor_table", "neighbor_rows", "NavigationGraph"):
        assert name in dllm.__all__ and callable(getattr(dllm, name))
    assert dllm.search.neighbor_rows is dllm.neighbor_rows
    for name in ("neighbors", "build_graph"):
        assert callable(getattr(dllm.VectorIndex, name))


def test_graph_block_keeps_the_workspace_under_the_budget(dllm):
    L = dllm._lib.load()
    for n, k in [(1, 1), (300, 10), (65536, 10), (1 << 20, 256), (5000, 256)]:
        b = dllm.search.graph_block(n, k)
        assert 1 <= b <= n
        assert b == 1 or L.dllm_neighbor_workspace(b, n, k) <= dllm.search.GRAPH_WORKSPACE_BUDGET
        assert b == n or L.dllm_neighbor_workspace(2 * b + 2, n, k) > dllm.search.GRAPH_WORKSPACE_BUDGET


def test_navigation_graph_bookkeeping(dllm):
    """NavigationGraph over plain CPU tensors: ids map rows, -1 places are no edges."""
    import torch
    idx = torch.tensor([[2, 1], [0, -1], [-1, -1]], dtype=torch.int32)
    sc = torch.tensor([[0.9, 0.85], [0.85, -math.inf], [-math.inf, -math.inf]], dtype=torch.float32)
    g = dllm.NavigationGraph([70, 30, 110], idx, sc)
    assert len(g) == 3 and g.ids == [70, 30, 110]
    assert g.neighbors(70) == [(110, pytest.approx(0.9)), (30, pytest.approx(0.85))]
    assert g.neighbors(30) == [(70, pytest.approx(0.85))] and g.neighbors(110) == [] and g.neighbors(5) == []
    assert [(a, b) for a, b, _ in g.edges()] == [(70, 110), (70, 30), (30, 70)]


def test_vector_index_graph_calls_with_device_stubbed(dllm, monkeypatch):
    """build_graph walks the store in blocks with self_base = the block's first row and slices of one
    cached pair table; neighbors() uses the id's row and the same cached table."""
    import torch
    calls, tables = [], []

    def fake_table(codes, scales, zps):
        tables.append(codes.shape[0])
        return torch.zeros(codes.shape[0], 24, dtype=torch.uint8)

    def fake_rows(qc, qs, qz, c, s, z, k, threshold=NINF, self_base=-1, qtable=None, table=None):
        calls.append((qc.shape[0], c.shape[0], k, threshold, self_base, qtable.shape[0], table.shape[0]))
        nq = qc.shape[0]
        idx = ((torch.arange(nq)[:, None] + self_base + 1 + torch.arange(k)[None, :]) % c.shape[0]).to(torch.int32)
        return idx, torch.full((nq, k), 0.5)

    monkeypatch.setattr(dllm.search, "neighbor_table", fake_table)
    monkeypatch.setattr(dllm.search, "neighbor_rows", fake_rows)
    ix = dllm.VectorIndex(4, 8)
    ix._assign([10, 20, 30, 40, 50, 60, 70])
    ix._codes = torch.zeros(64, 4, dtype=torch.uint8)
    ix._scales = ix._zps = torch.zeros(64)
    g = ix.build_graph(2, block=3)
    assert tables == [7]
    assert calls == [(3, 7, 2, 0.8, 0, 3, 7), (3, 7, 2, 0.8, 3, 3, 7), (1, 7, 2, 0.8, 6, 1, 7)]
    assert g.ids == [10, 20, 30, 40, 50, 60, 70] and tuple(g.idx.shape) == (7, 2)
    assert g.neighbors(70) == [(10, 0.5), (20, 0.5)]
    calls.clear()
    got = ix.neighbors([30, 99], 2, threshold=0.1)
    assert tables == [7]                                   # the cached table
    assert calls == [(1, 7, 2, 0.1, 2, 1, 7)]
    assert got == [[(40, 0.5), (50, 0.5)], []]
    g2 = ix.build_graph(1)                                 # the default block: one call for a small store
    assert calls[-1] == (7, 7, 1, 0.8, 0, 7, 7) and len(g2) == 7
    with pytest.raises(dllm.InvalidParams):
        ix.build_graph(0)
    with pytest.raises(dllm.InvalidParams):
        ix.build_graph(2, block=0)
    with pytest.raises(dllm.InvalidParams):
        ix.neighbors([10], 257)


# ---- the host entry points under the sanitizers -----------------------------------------------------

def test_host_entry_points_under_sanitizers(tmp_path):
    """tests/cpp/neighbors_host_check.cpp (its own main) with csrc/host_rules.cpp and error.cpp, compiled by
    g++ under the address and undefined-behaviour sanitizers (tests/host_check.py; no hipcc, no
    library): exact-size heap buffers at every kind of dim, blocks from the start, middle and end."""
    run_host_check("neighbors_host_check", tmp_path, timeout=120)
